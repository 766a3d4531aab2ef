"""The reference of the sphere step moves (include/bge_world.h "Sphere step moves"): step_ref, the header's rule in numpy float32
scalars (written from the header, not from the kernel) over a caster handed in — the casters are those of refmodel/moves.py — and
compose_ref, the same result put together from the public pieces the header names (a cast up, a plain move with probe 0, a cast
down, a probe)."""
from __future__ import annotations

import numpy as np

from .records import MOVE_GROUNDED, MOVE_INVALID, MOVE_OUT_OF_SLIDES, MOVE_PROBE_HIT, MOVE_SLIDES, SPHERE_CAST_DTYPE
from .rays import NO_ENTITY, RAY_MISS
from .moves import F, MIN_APPROACH, REST_SQ, _dot, move_ref, mover_valid

STEP_TRIED, STEPPED = 16, 32
STEP_MOVE_DTYPE = np.dtype([("position", "<f4", (3,)), ("displacement", "<f4", (3,)), ("radius", "<f4"), ("skin", "<f4"),
                            ("probe_distance", "<f4"), ("min_ground_ny", "<f4"), ("layer_mask", "<u4"), ("step_height", "<f4")])
STEP_RESULT_DTYPE = np.dtype([("position", "<f4", (3,)), ("remaining", "<f4", (3,)), ("flags", "<u4"), ("n_hits", "<u4"),
                              ("hit_kind", "<u4"), ("hit_entity", "<u4"), ("hit_normal", "<f4", (3,)), ("ground_kind", "<u4"),
                              ("ground_entity", "<u4"), ("ground_distance", "<f4"), ("ground_normal", "<f4", (3,)), ("step_rise", "<f4")])
# the plain move's records over the same bytes
PLAIN_MOVE_DTYPE = np.dtype([(n, STEP_MOVE_DTYPE.fields[n][0]) if n != "step_height" else ("reserved", "<u4") for n in STEP_MOVE_DTYPE.names])
# what a mover came to, for the coverage of the seeded batches
OUTCOMES = ("invalid", "free", "gate closed", "no rise", "down miss", "steep landing", "no gain", "stepped")

ZERO = [F(0), F(0), F(0)]


def step_mover_valid(m):
    with np.errstate(all="ignore"):
        return bool(mover_valid(m) and np.isfinite(m["step_height"]) and m["step_height"] >= 0)


class _Slide:
    """Slide(p, d) for the movers of `active`: rounds 1-7 of "Sphere moves" for MOVE_SLIDES rounds, r = d0 = d, no previous normal."""

    def __init__(self, cast_fn, moves, start, disp, active):
        n = len(moves)
        self.p = [[F(v) for v in s] for s in start]
        r = [[F(v) for v in d] if active[i] else list(ZERO) for i, d in enumerate(disp)]
        d0 = [list(v) for v in r]
        prev = [None] * n
        done = [not a for a in active]
        self.n_hits = [0] * n
        self.last = [None] * n  # (kind, entity, normal) of the last hit
        self.n1 = [None] * n    # the normal of the first round's hit
        p = self.p
        for rnd in range(MOVE_SLIDES):
            casts = np.zeros(n, SPHERE_CAST_DTYPE)
            L2 = [None] * n
            for i in range(n):
                if done[i]:
                    continue
                L2[i] = _dot(r[i], r[i])
                if not L2[i] > REST_SQ:  # 1
                    r[i], done[i] = list(ZERO), True
                    continue
                casts[i] = (p[i], r[i], 1.0, moves["radius"][i], moves["layer_mask"][i], 0)
            hits = cast_fn(casts)
            for i in range(n):
                if done[i]:
                    continue
                h = hits[i]
                if h["kind"] == RAY_MISS:  # 2
                    p[i] = [p[i][j] + r[i][j] for j in range(3)]
                    r[i], done[i] = list(ZERO), True
                    continue
                f, nrm, skin = F(h["fraction"]), [F(v) for v in h["normal"]], F(moves["skin"][i])
                L = np.sqrt(L2[i])  # 3
                a = -(_dot(r[i], nrm) / L)
                if not a >= MIN_APPROACH:
                    a = MIN_APPROACH
                g = f - skin / (a * L)
                if not g > 0:
                    g = F(0)
                p[i] = [p[i][j] + r[i][j] * g for j in range(3)]
                self.n_hits[i] += 1
                self.last[i] = (h["kind"], h["entity"], nrm)
                if rnd == 0:
                    self.n1[i] = nrm
                w = F(1) - f  # 4
                lft = [r[i][j] * w for j in range(3)]
                dn = _dot(lft, nrm)
                s = [lft[j] - nrm[j] * dn for j in range(3)]
                m = prev[i]
                if m is not None and _dot(s, m) < 0:  # 5
                    c = [m[1] * nrm[2] - m[2] * nrm[1], m[2] * nrm[0] - m[0] * nrm[2], m[0] * nrm[1] - m[1] * nrm[0]]
                    cc = _dot(c, c)
                    if not cc > REST_SQ:
                        s = list(ZERO)
                    else:
                        t = _dot(lft, c) / cc
                        s = [c[j] * t for j in range(3)]
                if not _dot(s, d0[i]) > 0:  # 6
                    s = list(ZERO)
                r[i], prev[i] = s, nrm  # 7
        self.out_of_slides = [bool(_dot(v, v) > REST_SQ) for v in r]
        self.r = [v if o else list(ZERO) for v, o in zip(r, self.out_of_slides)]

    def fill(self, out, i):
        out["remaining"][i] = self.r[i]
        if self.out_of_slides[i]:
            out["flags"][i] |= MOVE_OUT_OF_SLIDES
        out["n_hits"][i] = self.n_hits[i]
        if self.last[i] is not None:
            out["hit_kind"][i], out["hit_entity"][i], out["hit_normal"][i] = self.last[i]


def _cast_one_way(cast_fn, moves, origins, dy, dist, ask):
    casts = np.zeros(len(moves), SPHERE_CAST_DTYPE)
    for i in range(len(moves)):
        if ask[i]:
            casts[i] = (origins[i], (0.0, dy, 0.0), dist[i], moves["radius"][i], moves["layer_mask"][i], 0)
    return cast_fn(casts)


def step_ref(cast_fn, moves, trace=None):
    """The header's rule.  cast_fn(casts: SPHERE_CAST_DTYPE[n]) -> RAY_HIT_DTYPE[n] answers one pass (layer_mask 0 asks nothing).
    trace, if a dict, gets per mover "outcome" (one of OUTCOMES), "capped" (whether the Up cast hit) and "landing" (the kind of the
    Down hit the step would land on, RAY_MISS if it did not get there)."""
    n = len(moves)
    out = np.zeros(n, STEP_RESULT_DTYPE)
    out["hit_entity"] = NO_ENTITY
    out["ground_entity"] = NO_ENTITY
    outcome = ["invalid"] * n
    capped = np.zeros(n, bool)
    landing = np.full(n, RAY_MISS)
    with np.errstate(all="ignore"):
        valid = [step_mover_valid(m) for m in moves]
        pos = [[F(v) for v in m["position"]] for m in moves]
        disp = [[F(v) for v in m["displacement"]] for m in moves]
        skin, probe, min_ny = moves["skin"], moves["probe_distance"], moves["min_ground_ny"]
        # Plain
        P = _Slide(cast_fn, moves, pos, disp, valid)
        # Gate
        tried = [bool(valid[i] and moves["step_height"][i] > 0 and P.n_hits[i] >= 1 and P.n1[i][1] < F(min_ny[i])
                      and disp[i][0] * disp[i][0] + disp[i][2] * disp[i][2] > REST_SQ) for i in range(n)]
        for i in range(n):
            if valid[i]:
                outcome[i] = "gate closed" if P.n_hits[i] >= 1 else "free"
        # Up
        hits = _cast_one_way(cast_fn, moves, pos, 1.0, moves["step_height"], tried)
        u = [F(0)] * n
        alive = list(tried)
        for i in range(n):
            if not tried[i]:
                continue
            u[i] = F(moves["step_height"][i])
            if hits[i]["kind"] != RAY_MISS:
                u[i] = F(hits[i]["distance"]) - F(skin[i])
                capped[i] = True
            if not u[i] > 0:
                alive[i], outcome[i] = False, "no rise"
        q = [[pos[i][0], pos[i][1] + u[i], pos[i][2]] for i in range(n)]
        # Forward
        Fw = _Slide(cast_fn, moves, q, [[d[0], F(0), d[2]] for d in disp], alive)
        # Down
        m = [u[i] + F(probe[i]) for i in range(n)]
        hits = _cast_one_way(cast_fn, moves, Fw.p, -1.0, m, alive)
        S = [None] * n
        for i in range(n):
            if not alive[i]:
                continue
            h = hits[i]
            if h["kind"] == RAY_MISS:
                alive[i], outcome[i] = False, "down miss"
            elif not F(h["normal"][1]) >= F(min_ny[i]):
                alive[i], outcome[i] = False, "steep landing"
            else:
                e = F(h["distance"]) - F(skin[i])
                if not e > 0:
                    e = F(0)
                S[i] = [Fw.p[i][0], Fw.p[i][1] - e, Fw.p[i][2]]
                landing[i] = h["kind"]
                # Gain
                gs = (S[i][0] - pos[i][0]) * disp[i][0] + (S[i][2] - pos[i][2]) * disp[i][2]
                gp = (P.p[i][0] - pos[i][0]) * disp[i][0] + (P.p[i][2] - pos[i][2]) * disp[i][2]
                if not gs > gp:
                    alive[i], outcome[i] = False, "no gain"
        # Result
        chosen = [None] * n
        for i in range(n):
            if not valid[i]:
                out["flags"][i] = MOVE_INVALID
                out["position"][i] = moves["position"][i]
                chosen[i] = pos[i]
                continue
            if tried[i]:
                out["flags"][i] |= STEP_TRIED
            if alive[i]:
                outcome[i] = "stepped"
                out["flags"][i] |= STEPPED
                chosen[i] = S[i]
                Fw.fill(out, i)
                out["step_rise"][i] = u[i]
            else:
                chosen[i] = P.p[i]
                P.fill(out, i)
            out["position"][i] = chosen[i]
        # Probe
        asks = [bool(valid[i] and probe[i] > 0) for i in range(n)]
        hits = _cast_one_way(cast_fn, moves, chosen, -1.0, probe, asks)
        for i in range(n):
            h = hits[i]
            if asks[i] and h["kind"] != RAY_MISS:
                out["flags"][i] |= MOVE_PROBE_HIT
                out["ground_kind"][i], out["ground_entity"][i], out["ground_distance"][i] = h["kind"], h["entity"], h["distance"]
                out["ground_normal"][i] = h["normal"]
                if F(h["normal"][1]) >= F(min_ny[i]):
                    out["flags"][i] |= MOVE_GROUNDED
    if trace is not None:
        trace["outcome"], trace["capped"], trace["landing"] = outcome, capped, landing
    return out


def plain_of(moves):
    """The same 48 bytes read as bge_sphere_move records."""
    return np.ascontiguousarray(moves).view(PLAIN_MOVE_DTYPE)


def compose_ref(cast_fn, moves, got, move_fn=None):
    """What the header's consequences promise for the records `got` of `moves`, from the public pieces: where STEPPED is not set,
    the plain move of the same bytes (got has STEP_TRIED in addition); where it is, one cast up, a plain move with probe 0 from
    the raised position by the level displacement, one cast down, one probe.  move_fn(plain moves) -> plain results is the plain
    move (move_ref on cast_fn if None).  Returns the records as STEP_RESULT_DTYPE, with got's STEP_TRIED bit."""
    if move_fn is None:
        move_fn = lambda mv: move_ref(cast_fn, mv)  # noqa: E731
    n = len(moves)
    plain = move_fn(plain_of(moves))
    want = np.ascontiguousarray(plain).view(STEP_RESULT_DTYPE).copy()  # (the reserved word 0 reads as step_rise 0)
    want["flags"] |= got["flags"] & STEP_TRIED
    for i in range(n):  # (a step_height that is not a height invalidates a mover the plain move accepts)
        if not step_mover_valid(moves[i]) and not (plain["flags"][i] & MOVE_INVALID):
            want[i] = np.zeros(1, STEP_RESULT_DTYPE)[0]
            want["position"][i], want["flags"][i], want["hit_entity"][i], want["ground_entity"][i] = moves["position"][i], MOVE_INVALID, NO_ENTITY, NO_ENTITY
    st = np.nonzero((got["flags"] & STEPPED) != 0)[0]
    if len(st) == 0:
        return want
    mv = moves[st]
    with np.errstate(all="ignore"):
        up = _cast_one_way(cast_fn, mv, mv["position"], 1.0, mv["step_height"], [True] * len(st))
        u = np.where(up["kind"] == RAY_MISS, mv["step_height"], (up["distance"] - mv["skin"]).astype(np.float32)).astype(np.float32)
        fwd = plain_of(mv).copy()
        fwd["position"][:, 1] = mv["position"][:, 1] + u
        fwd["displacement"][:, 1] = 0
        fwd["probe_distance"] = 0
        fwd["reserved"] = 0
        fr = move_fn(fwd)
        m = (u + mv["probe_distance"]).astype(np.float32)
        down = _cast_one_way(cast_fn, mv, fr["position"], -1.0, m, [True] * len(st))
        e = (down["distance"] - mv["skin"]).astype(np.float32)
        e = np.where(e > 0, e, np.float32(0)).astype(np.float32)
        S = fr["position"].copy()
        S[:, 1] = fr["position"][:, 1] - e
        probe = _cast_one_way(cast_fn, mv, S, -1.0, mv["probe_distance"], list(mv["probe_distance"] > 0))
    for k, i in enumerate(st):
        assert down["kind"][k] != RAY_MISS and down["normal"][k][1] >= mv["min_ground_ny"][k] and u[k] > 0, (i, "the composition does not land")
        rec = np.zeros(1, STEP_RESULT_DTYPE)
        for name in ("remaining", "n_hits", "hit_kind", "hit_entity", "hit_normal"):
            rec[name][0] = fr[name][k]
        rec["position"][0] = S[k]
        rec["flags"][0] = (fr["flags"][k] & MOVE_OUT_OF_SLIDES) | STEP_TRIED | STEPPED
        rec["ground_entity"][0] = NO_ENTITY
        rec["step_rise"][0] = u[k]
        h = probe[k]
        if mv["probe_distance"][k] > 0 and h["kind"] != RAY_MISS:
            rec["flags"][0] |= MOVE_PROBE_HIT
            rec["ground_kind"][0], rec["ground_entity"][0], rec["ground_distance"][0], rec["ground_normal"][0] = h["kind"], h["entity"], h["distance"], h["normal"]
            if h["normal"][1] >= mv["min_ground_ny"][k]:
                rec["flags"][0] |= MOVE_GROUNDED
        want[i] = rec[0]
    return want
