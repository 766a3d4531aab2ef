// path_epochs — bge::PathEpochs (csrc/bge_epochs.hpp) on its own: what moves which epoch, and the wrap rule.
#include <cstdio>
#include <cstdlib>

#include "bge_epochs.hpp"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            return 1;                                                   \
        }                                                               \
    } while (0)

int main()
{
    bge::PathEpochs e;
    CHECK(e.rows == 1 && e.rest == 1);
    // a host edit moves both, every time
    unsigned rows_bumps = 0, rest_bumps = 0;
    for (int k = 0; k < 1000; ++k) {
        const uint32_t r0 = e.rows, s0 = e.rest;
        CHECK(!e.host_edit());
        rows_bumps += e.rows != r0;
        rest_bumps += e.rest != s0;
    }
    CHECK(rows_bumps == 1000 && rest_bumps == 1000);
    // a tick without one path moves that path's epoch alone
    uint32_t r0 = e.rows, s0 = e.rest;
    CHECK(!e.tick_without_rows());
    CHECK(e.rows == r0 + 1 && e.rest == s0);
    CHECK(!e.tick_without_rest());
    CHECK(e.rows == r0 + 1 && e.rest == s0 + 1);
    // wrap: never 0 (0 means "path off" to the kernel), and reported so that the caller zeroes the words
    e.rows = 0xffffffffu;
    e.rest = 7;
    CHECK(e.tick_without_rows());
    CHECK(e.rows == 1 && e.rest == 7);
    e.rest = 0xffffffffu;
    CHECK(e.tick_without_rest());
    CHECK(e.rest == 1);
    e.rows = 0xffffffffu;
    e.rest = 5;
    CHECK(e.host_edit()); // one of the two wrapped
    CHECK(e.rows == 1 && e.rest == 6);
    e.rows = 5;
    e.rest = 0xffffffffu;
    CHECK(e.host_edit());
    CHECK(e.rows == 6 && e.rest == 1);
    std::printf("path_epochs ok\n");
    return 0;
}
