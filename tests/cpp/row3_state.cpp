// row3_state — bge::Row3State (csrc/bge_epochs.hpp) on its own, next to bge::PathEpochs: when a tick may defer the translation row,
// when a store (k_row3_sync) is due and with which epoch, and what pinning does.
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
    bge::Row3State r;
    // nothing is due before a deferring tick, and asking twice changes nothing
    CHECK(r.pending == 0 && !r.pinned);
    CHECK(r.take_sync() == 0 && r.take_sync() == 0);
    // who may defer: a translation-row tick of a scene with one pass and no frozen root, unless switched off
    CHECK(r.may_defer(true, 1, false, true));
    CHECK(!r.may_defer(false, 1, false, true)); // no translation-row path in this tick
    CHECK(!r.may_defer(true, 2, false, true));  // a later pass reads stored matrices
    CHECK(!r.may_defer(true, 0, false, true));  // an empty layout
    CHECK(!r.may_defer(true, static_cast<size_t>(0) - 1, false, true)); // (pass_tile_begin.size() - 1 of an empty vector)
    CHECK(!r.may_defer(true, 1, true, true));   // a frozen root reads its stored matrix
    CHECK(!r.may_defer(true, 1, false, false)); // BGE_DEFER_ROW3=0
    // deferring ticks under one rows epoch: one store is due, with that epoch, however many ticks ran
    for (int k = 0; k < 5; ++k) r.deferred(e.rows);
    CHECK(r.pending == e.rows);
    const uint32_t before = e.rows;
    CHECK(r.take_sync() == before); // the caller launches k_row3_sync(before) here: BEFORE the epoch moves
    CHECK(!e.host_edit());
    CHECK(e.rows == before + 1);
    CHECK(r.pending == 0 && r.take_sync() == 0); // nothing more is due
    // the same in front of a tick without the translation-row path
    r.deferred(e.rows);
    CHECK(r.take_sync() == e.rows);
    CHECK(!e.tick_without_rows());
    CHECK(r.take_sync() == 0);
    // readers compose with `pending` as their epoch: 0 (never a live epoch) composes nothing
    CHECK(bge::PathEpochs{}.rows != 0 && bge::PathEpochs{}.rest != 0);
    e.rows = 0xffffffffu;
    CHECK(e.tick_without_rows() && e.rows == 1); // (the wrap never hands out 0 either)
    // pinning: what is deferred is still due once, and no tick defers again
    r.deferred(e.rows);
    r.pinned = true;
    CHECK(r.take_sync() == e.rows);
    CHECK(!r.may_defer(true, 1, false, true));
    CHECK(r.take_sync() == 0);
    std::printf("row3_state ok\n");
    return 0;
}
