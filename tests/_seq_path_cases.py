"""Directed contention cases for the sequential engine's in-order validator
(ms_seq.hip: validate_batch, walk_top4, validate_scan, merge_pod_lists), with a
structural model of its routes in Python integers.

The random clusters of the parity tests decide which route resolves a pod by
the draw. Here a table has a handful of feasible "hot" rows and a whole batch
contends for them; every other ("cold") row is rejected statically:
  cordon  unschedulable and full: NodeUnschedulable for a pod that does not
          tolerate it, NodeResourcesFit for one that does
  full    allowed_pods == pod_count: NodeResourcesFit
  nocpu   alloc_milli_cpu == 0: NodeResourcesFit for a pod that requests CPU
          (cases whose pods all request; feasible otherwise)
  gone    tombstoned: no filter sees it
Tiles are 64..256 rows (a multiple of 16, from the CU count), so rows within an
aligned 16-row block share a tile and rows >= 256 apart never do, whatever the
size; a block at row >= 16,384 has a tile index >= 64.

Plateau tables: hot rows of 10^9 m / 2^40 B and pods without requests (non-zero
defaults 100 m / 200 MiB) keep a hot row's LeastAllocated score at 99 for its
first 51 binds, so a (pod, row) key is the same whatever earlier binds a sweep
saw; plateau_ok() asserts it from the integer formula.

Two models, both from the oracle's placements and the host's batch boundaries:
  classify()   per pod, the class of the issue's structural rule, from the
               batch-start lists and the rows bound by EARLIER PODS OF THE SAME
               BATCH: fast, walk, ext, scan (+ tiles to re-sweep), and the
               FitError routes spec / round / scan
  simulate()   the validator's rounds restated step by step (claims with the
               kernel's claim hash, the 16-pod walks, the serial pod, the list
               scan): the exact counters of a batch whose stale set is known,
               i.e. every batch here (the filler pods bind nothing)
Test infrastructure, never product code.
"""
from __future__ import annotations

import numpy as np

import _la_cases as lc

N_NODES = 19_996       # no tile size divides it: the last tile is short at every size
SEED = 7
ORD0 = 4096          # first pod ordinal of every case
WARM_PODS, WARM_BATCH, FULL_BATCH = 4096, 64, 128   # ms_seq_host.cpp kWarmPods, kWarmBatch, kSeqBatch
TILE_ROWS = tuple(range(64, 257, 16))
HOT_CPU, HOT_MEM = 10**9, 1 << 40
NZ_CPU, NZ_MEM = 100, 200 << 20
PLATEAU_BINDS = 51
TOPK, TOPEXT = 4, 8
CLASSES = ("fast", "walk", "ext", "scan")
FIT_ROUTES = ("fit_spec", "fit_round", "fit_scan")
MASK_NU, MASK_NRF = 1, 2
CODE_SUCCESS, CODE_ERROR, CODE_UNSCHEDULABLE = 0, 1, 2


def tile_rows_for(rows, cus):
    """run_sequential's tile size: one tile per CU beside the validator's."""
    room = max(2, cus) - 1
    tr = (-(-rows // room) + 15) // 16 * 16
    return min(256, max(64, tr))


def batches(n_pods, full=FULL_BATCH):
    """(first pod, count) of every speculative batch of one call (batch_at)."""
    out, s0 = [], 0
    while s0 < n_pods:
        nb = min(WARM_BATCH if s0 < WARM_PODS else full, n_pods - s0)
        out.append((s0, nb))
        s0 += nb
    return out


def claim_hash(row):
    return ((row * 0x85EBCA6B) & 0xFFFFFFFF) >> 20


# ---- cases -----------------------------------------------------------------------
class Case:
    """name; hot: {row: room for pods}; cold: the cold rows' reasons, cycled by row;
    n: directed pods; filler: 4,096 unplaceable pods first (128-pod batches after
    them); plateau: the plateau table (else rows of 1000 m / 2 GiB and requesting
    pods); tol / nodigit: every tol-th directed pod tolerates, every nodigit-th has
    no name digit; want: the classes and routes the case is named for; by_tile:
    hot rows given as a function of the tile size; digit: (the directed pods' name
    digit, {hot row: name digit}) where NodeNumber is to rank the hot rows; decoy: cold rows
    (cordoned and full) given a capacity of 2^41, outside the binary64 sweep's range,
    so that their tiles are swept lane = row with exact per-row filter flags."""

    def __init__(self, name, hot, n=64, cold=("full", "gone", "cordon"), filler=False, plateau=True, tol=0, nodigit=0,
                 want=(), by_tile=None, bounds=True, digit=None, decoy=()):
        self.name, self.n, self.cold, self.filler, self.plateau = name, n, tuple(cold), filler, plateau
        self.tol, self.nodigit, self.want, self.by_tile, self.bounds = tol, nodigit, tuple(want), by_tile, bounds
        self._hot, self.digit, self.decoy = hot, digit, tuple(decoy)

    def hot(self, tile_rows):
        h = self.by_tile(tile_rows) if self.by_tile else self._hot
        return dict(h) if isinstance(h, dict) else {r: 60 for r in h}


def block(row0, k, step=1):
    return [row0 + step * i for i in range(k)]


def spread(k, row0=300, step=1200):
    """k rows at least 256 apart (one per tile at every tile size), not aligned to a tile."""
    return [row0 + step * i + 3 * (i % 5) for i in range(k)]


LAST_BLOCK = N_NODES // 16 * 16   # row 19,984: in the short last tile at every tile size
assert all(LAST_BLOCK // tr == (N_NODES - 1) // tr and N_NODES % tr for tr in TILE_ROWS)

CASES = [
    Case("block6_hi", block(19_008, 6), want=("fast", "scan", "resweep")),
    Case("block6_hi_2x128", block(19_008, 6), n=256, filler=True, want=("scan", "resweep")),
    Case("spread8", spread(8), want=("walk", "scan"), cold=("full", "cordon")),
    Case("spread6_list_ends", spread(6), want=("walk", "ext"), cold=("gone", "full")),
    Case("spread12", spread(12), want=("walk", "ext", "scan")),
    Case("block5_spread4", block(4_112, 5) + spread(4, 9_000), want=("scan", "resweep")),
    Case("two_blocks5", block(2_064, 5) + block(17_424, 5), want=("walk", "scan", "resweep")),
    Case("block6_last_tile_room3", {r: 3 for r in block(LAST_BLOCK + 5, 6)}, want=("scan", "resweep", "fit_scan"),
         cold=("cordon", "full")),
    # two full blocks on one lane (tiles t and t + 64) and on two lanes
    Case("blocks_same_lane", None, by_tile=lambda tr: block(3 * tr + 16, 4) + block(67 * tr + 16, 4), n=128,
         filler=True, want=("scan", "resweep")),
    Case("blocks_two_lanes", block(1_040, 4) + block(3_088, 4), want=("scan", "resweep")),
    # more than 16 pods walking in one round: 40 rows one per tile, short lists never full
    Case("spread40_many_walkers", spread(40, 100, 400), n=128, filler=True, want=("walk",)),
    Case("nodigit_among", block(8_208, 6), nodigit=3, want=("scan", "resweep")),
    # a listed entry outside the certified ranks: a full block of 5 cuts the certified ranks
    # at 4 or 5; a second tile lists two rows, the first matching every pod's digit (109) and
    # the other not (99: always last, never bound). A scanning pod whose winner is the first
    # re-evaluates it and then meets the untouched second one, which must not replace it
    Case("block5_pair_low", block(10_256, 5) + block(13_328, 2), want=("scan", "resweep"),
         digit=(3, {**{r: 3 for r in block(10_256, 5)}, 13_328: 3, 13_329: 4})),
    # exhaustion: cordoned cold rows beside pods that do and do not tolerate them
    Case("spread3_room2_masks", {r: 2 for r in spread(3)}, cold=("cordon",), tol=4, want=("walk", "fit_round")),
    Case("block6_room3_masks", {r: 3 for r in block(12_304, 6)}, cold=("cordon", "gone"), tol=3,
         want=("scan", "fit_scan")),
    # the transposed sweep flags NodeResourcesFit on every tile that holds a row neither absent
    # nor NodeUnschedulable-rejected, a feasible one included; the lane = row sweep flags
    # rejections only. A 2^41 decoy puts the hot tile on the lane = row sweep, so the scan
    # route's NodeResourcesFit bit can only come from the tile's own listed rows
    Case("block6_room3_general_tile", {r: 3 for r in block(14_352, 6)}, cold=("cordon", "gone"), tol=3,
         decoy=(14_358,), want=("scan", "fit_scan")),
    Case("filler_then_block6", block(19_008, 6), n=128, filler=True, want=("fit_spec", "scan", "resweep")),
    # non-plateau: every bind moves the score by whole steps. One batch at the start of a
    # context (its lists saw no bind: counters as exact as on the plateau), and three
    # batches whose sweeps may or may not have seen the batch before (parity only)
    Case("steps_block6", block(6_160, 6), plateau=False, cold=("nocpu", "full", "cordon"), want=("scan", "resweep")),
    Case("steps_three_batches", spread(5) + block(15_376, 5), n=192, plateau=False, cold=("nocpu", "gone"), bounds=False),
]
CASE = {c.name: c for c in CASES}


def build(case, node_rec, pod_rec, tile_rows=80):
    """(node records, tombstoned rows, pod records, index of the first directed pod).
    The oracle takes the records with allowed_pods = -1 on the tombstoned rows."""
    hot = case.hot(tile_rows)
    assert all(0 <= r < N_NODES for r in hot)
    nodes = np.zeros(N_NODES, dtype=node_rec)
    rows = np.arange(N_NODES)
    reason = np.array(case.cold)[rows % len(case.cold)]
    nodes["name_digit"] = np.where(rows % 11 == 10, 0xFF, rows % 10)
    nodes["alloc_milli_cpu"], nodes["alloc_memory"] = 4000, 8 << 30
    nodes["allowed_pods"] = 110
    full = (reason == "full") | (reason == "cordon")
    nodes["pod_count"][full] = 110
    nodes["unschedulable"][reason == "cordon"] = 1
    nodes["alloc_milli_cpu"][reason == "nocpu"] = 0
    gone = np.nonzero(reason == "gone")[0]
    hr = np.array(sorted(hot))
    gone = np.setdiff1d(gone, hr)
    nodes["unschedulable"][hr] = 0
    nodes["pod_count"][hr] = 7
    nodes["allowed_pods"][hr] = [7 + hot[r] for r in hr]
    if case.plateau:
        nodes["alloc_milli_cpu"][hr], nodes["alloc_memory"][hr] = HOT_CPU, HOT_MEM
    else:
        nodes["alloc_milli_cpu"][hr], nodes["alloc_memory"][hr] = 1000, 2 << 30
    for r in case.decoy:
        assert reason[r] == "cordon" and r not in hot
        nodes["alloc_milli_cpu"][r] = nodes["alloc_memory"][r] = lc.K_FAST_CAP
    n_fill = WARM_PODS if case.filler else 0
    pods = np.zeros(n_fill + case.n, dtype=pod_rec)
    pods["ordinal"] = ORD0 + np.arange(len(pods))
    pods["name_digit"] = pods["ordinal"] % 10
    pods["nonzero_milli_cpu"], pods["nonzero_memory"] = NZ_CPU, NZ_MEM
    # the filler: more than any row has, so nothing is feasible at speculation
    pods["req_milli_cpu"][:n_fill] = pods["nonzero_milli_cpu"][:n_fill] = 2 * HOT_CPU
    d = np.arange(case.n)
    if not case.plateau:  # requests of 30 m / 64 MiB: a step of LeastAllocated per bind or two
        pods["req_milli_cpu"][n_fill:] = pods["nonzero_milli_cpu"][n_fill:] = 30 + 5 * (d % 3)
        pods["req_memory"][n_fill:] = pods["nonzero_memory"][n_fill:] = (64 << 20) + (d % 4 << 20)
    if case.digit:
        pods["name_digit"][n_fill:] = case.digit[0]
        for r, dg in case.digit[1].items():
            nodes["name_digit"][r] = dg
    if case.tol:
        pods["tolerates_unschedulable"][n_fill:] = d % case.tol == 1
    if case.nodigit:
        pods["name_digit"][n_fill:][d % case.nodigit == 1] = -1
    return nodes, gone, pods, n_fill


def oracle_nodes(nodes, gone):
    x = nodes.copy()
    x["allowed_pods"][gone] = -1
    return x


# ---- the model --------------------------------------------------------------------
class Hot:
    """The hot rows' live records (everything else is never feasible)."""

    def __init__(self, nodes, rows):
        self.rec = {int(r): {k: int(nodes[k][r]) for k in ("alloc_milli_cpu", "alloc_memory", "req_milli_cpu",
                                                            "req_memory", "nonzero_milli_cpu", "nonzero_memory",
                                                            "allowed_pods", "pod_count", "name_digit")}
                    for r in rows}

    def key(self, pod, row, seed=SEED):
        """The packed key of (pod, row) against the row's live record (_pyref.key and
        _pyref.h32 through _la_cases.key_of, the integer LeastAllocated formula); 0: rejected."""
        n = self.rec[row]
        if not lc.fits(n, pod):
            return 0
        s = lc.pair_score((n["alloc_milli_cpu"], n["nonzero_milli_cpu"], int(pod["nonzero_milli_cpu"])),
                          (n["alloc_memory"], n["nonzero_memory"], int(pod["nonzero_memory"])),
                          lc.nn_score(pod["name_digit"], n["name_digit"]) if pod["name_digit"] >= 0 else 0)
        return lc.key_of(s, seed, pod["ordinal"], row)

    def bind(self, pod, row):
        n = self.rec[row]
        n["pod_count"] += 1
        for a, b in (("req_milli_cpu", "req_milli_cpu"), ("req_memory", "req_memory"),
                     ("nonzero_milli_cpu", "nonzero_milli_cpu"), ("nonzero_memory", "nonzero_memory")):
            n[a] += int(pod[b])


def row_of(key):
    return 0xFFFFF - (key & 0xFFFFF)


class Lists:
    """One pod's batch-start lists: per tile the top-4 keys (best first), the merged
    ranks 0..7 and the certified count (merge_pod_lists: the ranks after the one that
    pops a full list's fourth entry are not certified; never below 4)."""

    def __init__(self, keys, tile_rows):
        self.tiles = {}
        for k in sorted((k for k in keys if k), reverse=True):
            self.tiles.setdefault(row_of(k) // tile_rows, []).append(k)
        self.tiles = {t: v[:TOPK] for t, v in self.tiles.items()}
        merged = sorted((k for v in self.tiles.values() for k in v), reverse=True)[:TOPEXT]
        self.cert = TOPEXT
        for r, k in enumerate(merged):
            v = self.tiles[row_of(k) // tile_rows]
            if len(v) == TOPK and v[-1] == k:
                self.cert = r + 1
                break
        self.cert = max(self.cert, TOPK)
        self.ranks = merged + [0] * (TOPEXT - len(merged))


def classify(L, bound):
    """The structural class of one pod: (class, tiles to re-sweep, bound entries above
    the deciding one). `bound`: rows bound by earlier pods of the batch."""
    if L.ranks[0] == 0:
        return "fit_spec", 0, 0
    if row_of(L.ranks[0]) not in bound:
        return "fast", 0, 0
    for r in range(L.cert):
        if L.ranks[r] == 0 or row_of(L.ranks[r]) not in bound:
            return ("walk" if r < TOPK else "ext"), 0, r
    rs = sum(1 for v in L.tiles.values() if len(v) == TOPK and all(row_of(k) in bound for k in v))
    above = L.cert
    for v in L.tiles.values():
        for k in v:
            if row_of(k) not in bound:
                break
            above += 1
    return "scan", rs, above


class Counts(dict):
    def __missing__(self, k):
        return 0


def run_model(case, nodes, pods, o, tile_rows, full=FULL_BATCH, simulate=True):
    """Replays the oracle's placements batch by batch. Returns (classes, sim):
    classes: Counts of classify()'s classes (+ 'resweep', 'above', and the FitError
    pods split by route); sim: the validator's counters by simulate_batch (pods,
    slow, scan, resweep, recompute) and its FitError routes. The FitError route of
    classify() is decided by the class the pod had when nothing was feasible."""
    hot_rows = sorted(case.hot(tile_rows))
    H = Hot(nodes, hot_rows)
    cls, sim = Counts(), Counts()
    prev = set()
    for s0, nb in batches(len(pods), full):
        bp = pods[s0:s0 + nb]
        keys0 = [[H.key(p, r) for r in hot_rows] for p in bp]
        L = [Lists(k, tile_rows) for k in keys0]
        if simulate and any(l.ranks[0] for l in L):
            Hs = Hot(nodes, [])
            Hs.rec = {r: dict(v) for r, v in H.rec.items()}
            got = simulate_batch(bp, L, Hs, prev, tile_rows, hot_rows, sim)
            for j in range(nb):  # the restated validator decides as the oracle does
                want = int(o["node"][s0 + j]) if o["code"][s0 + j] == CODE_SUCCESS else -1 - int(o["code"][s0 + j])
                assert got[j] == want, (case.name, s0 + j, got[j], want)
        else:
            sim["pods"] += nb
            sim["fit_spec"] += nb
        bound = set()
        for j, p in enumerate(bp):
            c, rs, above = classify(L[j], bound)
            code, node = int(o["code"][s0 + j]), int(o["node"][s0 + j])
            if code == CODE_UNSCHEDULABLE:
                cls[{"fit_spec": "fit_spec", "scan": "fit_scan"}.get(c, "fit_round")] += 1
            if c != "fit_spec":
                cls[c] += 1
                cls["resweep"] += rs
                cls["above"] += above
            if code == CODE_SUCCESS:
                assert node in H.rec, (case.name, "a cold row won", s0 + j, node)
                if case.plateau:  # every bind leaves the key of (pod, row) as the lists hold it
                    assert H.key(p, node) == keys0[j][hot_rows.index(node)], (case.name, "plateau", s0 + j)
                H.bind(p, node)
                bound.add(node)
        prev = bound
    return cls, sim


def plateau_ok(case, nodes, pods, o, tile_rows=80):
    """No hot row of a plateau case takes more than PLATEAU_BINDS pods, and the score
    of a pod without requests on it is the same (99, + 10 on a digit match) before
    the first and after the last of them."""
    hot = case.hot(tile_rows)
    won = o["node"][o["code"] == CODE_SUCCESS]
    for r in hot:
        k = int((won == r).sum())
        assert k <= PLATEAU_BINDS, (case.name, r, k)
        for b in (0, PLATEAU_BINDS):
            s = lc.pair_score((HOT_CPU, b * NZ_CPU, NZ_CPU), (HOT_MEM, b * NZ_MEM, NZ_MEM), 0)
            assert s == 99, (b, s)
    assert lc.pair_score((HOT_CPU, (PLATEAU_BINDS + 1) * NZ_CPU, NZ_CPU),
                         (HOT_MEM, (PLATEAU_BINDS + 1) * NZ_MEM, NZ_MEM), 0) == 98
    d = pods[len(pods) - case.n:]
    assert not d["req_milli_cpu"].any() and not d["req_memory"].any()


# ---- the validator's rounds, restated --------------------------------------------------
def _resolve(entries, known, touched, ev, ctr):
    """walk_top4's rule on up to four entries (known[r]: the entry counts): touched
    entries re-evaluated (each counted), the first untouched or ending one closes the
    list. Returns (winner key, needs more: no untouched or ending entry)."""
    f, vals = None, []
    for r, e in enumerate(entries):
        if not known[r]:
            vals.append(None)
        elif e == 0:
            vals.append("end")
        elif row_of(e) in touched:
            ctr["recompute"] += 1
            vals.append(("t", ev(row_of(e))))
        else:
            vals.append(("u", e))
    for r, v in enumerate(vals):
        if v is not None and (v == "end" or v[0] == "u"):
            f = r
            break
    m = 0
    for r, v in enumerate(vals):
        if v is None or v == "end":
            continue
        if (f is None or r < f) or (r == f and v[0] == "u"):
            m = max(m, v[1])
    return m, f is None


def simulate_batch(bp, L, H, prev, tile_rows, hot_rows, ctr):
    """validate_batch on one batch: pods bp, their lists L, live records H (updated),
    prev: rows the previous batch bound (stale: touched from the start). Adds to ctr;
    returns per pod the node bound, or -1 - code."""
    n = len(bp)
    touched, bound = set(prev), {}
    out = [None] * n
    sk = [l.ranks[0] for l in L]
    force = [False] * n
    for p in range(n):  # the prologue's stale re-resolution
        if sk[p] and prev and row_of(sk[p]) in prev:
            m, more = _resolve(L[p].ranks[:TOPK], [True] * TOPK, touched, lambda r: H.key(bp[p], r), ctr)
            if not more and m:
                sk[p] = m
            else:
                force[p] = True
    ctr["pods"] += n

    def bind(p, row):
        H.bind(bp[p], row)
        touched.add(row)
        bound[row] = bound.get(row, 0) + 1

    def fit(p, route):
        ctr[route] += 1
        out[p] = -1 - CODE_UNSCHEDULABLE

    for g in range(0, n, 64):
        gn = min(64, n - g)
        cvalid, ck, need = [False] * gn, [0] * gn, [False] * gn
        i0 = 0
        while i0 < gn:
            walkers = []
            for l in range(i0, gn):
                p = g + l
                if sk[p] == 0 or cvalid[l]:
                    continue
                cvalid[l], ck[l], need[l] = True, 0, False
                srow = row_of(sk[p])
                if not force[p] and not (srow in touched and (srow not in prev or bound.get(srow, 0))):
                    ck[l] = sk[p]
                else:
                    walkers.append(l)
            ctr["max_walk"] = max(ctr["max_walk"], len(walkers))
            for l in walkers:
                p = g + l
                ck[l], need[l] = _resolve(L[p].ranks[:TOPK], [True] * TOPK, touched, lambda r: H.key(bp[p], r), ctr)
            for l in range(gn):  # (every lane still holding `need`, the decided serial pods too)
                p = g + l
                if need[l] and L[p].cert > TOPK:
                    m, more = _resolve(L[p].ranks[TOPK:], [TOPK + r < L[p].cert for r in range(TOPK)], touched,
                                       lambda r: H.key(bp[p], r), ctr)
                    ck[l], need[l] = max(ck[l], m), more
            claim = {}
            for l in range(i0, gn):
                p = g + l
                if sk[p] and not need[l] and ck[l] and bp[p]["name_digit"] >= 0:
                    h = claim_hash(row_of(ck[l]))
                    claim[h] = min(claim.get(h, l), l)
            s, serial = gn, False
            for l in range(i0, gn):
                p = g + l
                if not sk[p]:
                    continue
                lost = not need[l] and ck[l] and claim.get(claim_hash(row_of(ck[l])), gn) < l
                if lost:
                    cvalid[l] = False
                if (need[l] or lost) and s == gn:
                    s, serial = l, need[l]
            for l in range(i0, s):
                p = g + l
                if ck[l] == 0:
                    fit(p, "fit_round" if sk[p] else "fit_spec")
                elif bp[p]["name_digit"] < 0:
                    out[p] = -1 - CODE_ERROR
                else:
                    out[p] = row_of(ck[l])
            for l in range(i0, s):
                if out[g + l] >= 0:
                    bind(g + l, out[g + l])
            if s == gn:
                break
            if not serial:
                i0 = s
                continue
            p = g + s
            ctr["slow"] += 1
            C = L[p].cert
            stop = next((r for r in range(C) if L[p].ranks[r] == 0 or row_of(L[p].ranks[r]) not in touched), None)
            scanned = stop is None
            if not scanned:
                b = L[p].ranks[stop]
                for r in range(stop):
                    ctr["recompute"] += 1
                    b = max(b, H.key(bp[p], row_of(L[p].ranks[r])))
            else:
                ctr["scan"] += 1
                b, resweep = 0, []
                for t, v in sorted(L[p].tiles.items()):
                    for k, e in enumerate(v):
                        if row_of(e) not in touched:
                            b = max(b, e)
                            break
                        ctr["recompute"] += 1
                        b = max(b, H.key(bp[p], row_of(e)))
                        if k == TOPK - 1:
                            resweep.append(t)
                for t in resweep:
                    ctr["resweep"] += 1
                    b = max([b] + [H.key(bp[p], r) for r in hot_rows if r // tile_rows == t])
            if b == 0:
                fit(p, "fit_scan" if scanned else "fit_round")
            elif bp[p]["name_digit"] < 0:
                out[p] = -1 - CODE_ERROR
            else:
                out[p] = row_of(b)
                bind(p, out[p])
                for l in range(gn):
                    if cvalid[l] and ck[l] and row_of(ck[l]) == out[p]:
                        cvalid[l] = False
            i0 = s + 1
    return out


# ---- shared, never modified ---------------------------------------------------------
_CACHE = {}


def prepared(case, oracle, node_rec, pod_rec, tile_rows=80):
    """(nodes, tombstoned rows, pods, first directed pod, oracle outputs) of a case,
    computed once per session (per tile size only where the rows depend on it)."""
    k = (case.name, tile_rows if case.by_tile else 0)
    if k not in _CACHE:
        nodes, gone, pods, n_fill = build(case, node_rec, pod_rec, tile_rows)
        o = oracle.schedule(oracle_nodes(nodes, gone), pods, plugin_set=1, mode=1, seed=SEED)
        _CACHE[k] = (nodes, gone, pods, n_fill, o)
    return _CACHE[k]
