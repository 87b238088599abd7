"""Inputs of the explain tests, shared by the CPU file (which judges the reference
on them against the oracle) and the GPU file (which runs them). A case is the
dict tests/_explain_ref.py reads. Test infrastructure.

Family: every plugin set x table sizes T - 1, T, T + 1, 2 T + 37 (T = the explain
kernels' row tile) and 1, 2, 3, 4, 5, 63, 64, 65 (the TaintToleration closed
form's special entries 0..2 and the last; 64-lane waves) x 0 % and 90 %
tombstones x node_base 0 and 33,333, 40 pods each: both tolerations, all ten
digits and a non-digit name, then set-specific pods. Directed cases follow.
"""
from __future__ import annotations

import numpy as np

import _la_cases
import _nam_required_cases
from minisched_amd import _lib, synth

T = _lib.EXPLAIN_TILE
SIZES = (T - 1, T, T + 1, 2 * T + 37, 1, 2, 3, 4, 5, 63, 64, 65)
TOMBSTONES = (0, 90)
NODE_BASES = (0, 33_333)
N_PODS = 40
N_SETS = 6
FULL = (1 << 256) - 1
# raw NodeAffinity score by zone id under KAT_TERMS: 1 -> 30, 2 -> 120, 3 -> 250, 4 -> 101
KAT_TERMS = [(30, 0b01110, FULL), (90, 0b01100, FULL), (100, 0b01000, FULL), (30, 0b01000, FULL)]
R101_TERMS = [(100, 0b10000, FULL), (1, 0b10000, FULL)]
LA_CAPS = _la_cases.GENERAL_CAPS[2:] + _la_cases.HUGE_CAPS  # 2^45 and up: above 2^47, around 2^53, to 2^56


def base_pods(ps, seed):
    """40 pods: [0, 20) digit d = j % 10 without / with the toleration, 20 and 21
    non-digit names, the rest as synth draws them; the set's own fields random."""
    pr = synth.pods(N_PODS, seed=seed, resources=ps == 1, zones=ps == 2, taints=ps == 3,
                    term_sets=N_SETS if ps == 4 else 0)
    pr["name_digit"][:20] = np.arange(20) % 10
    pr["tolerates_unschedulable"][:20] = np.arange(20) // 10
    pr["name_digit"][20:22] = -1
    pr["tolerates_unschedulable"][20:22] = (0, 1)
    if ps == 1:
        pr["req_milli_cpu"][22] = pr["req_memory"][22] = 0  # a zero-request pod: only "Too many pods" rejects it
        pr["nonzero_milli_cpu"][22], pr["nonzero_memory"][22] = synth.DEFAULT_MILLI_CPU_REQUEST, synth.DEFAULT_MEMORY_REQUEST
        for k, (cap, nz, n) in enumerate(_la_cases.N100_PRODUCT[:4]):  # zero Fit requests, huge non-zero ones
            p = pr[23 + k]
            p["req_milli_cpu"] = p["req_memory"] = 0
            p["nonzero_milli_cpu"] = p["nonzero_memory"] = n
    if ps == 4:
        pr["pref_zone"][22], pr["pref_weight"][22] = 0, 0              # set id 0: no terms
        pr["pref_zone"][23], pr["pref_weight"][23] = N_SETS + 5, 0     # an id above n_sets: no terms either
        pr["pref_zone"][24], pr["pref_weight"][24] = 1, 1              # id 257: far above
    return pr


def base_nodes(ps, n, seed):
    nr = synth.nodes(n, seed=seed, resources=ps == 1, zones=ps == 2, taints=ps == 3, labels=ps == 4)
    i = np.arange(n)
    nr["name_digit"][i % 7 == 3] = 0xFF  # non-digit node names
    if ps == 0 and seed % 2:
        nr["name_digit"] = ((i * 3 + 1) % 10).astype(np.uint8)  # digits off the ordinal: a misaligned group
        nr["name_digit"][i % 7 == 3] = 0xFF
    if ps == 1:
        # rows failing NodeResourcesFit on pods, on cpu and on memory
        nr["pod_count"][i % 11 == 1] = nr["allowed_pods"][i % 11 == 1]
        m = i % 11 == 2
        nr["req_milli_cpu"][m] = nr["nonzero_milli_cpu"][m] = nr["alloc_milli_cpu"][m]
        m = i % 11 == 3
        nr["req_memory"][m] = nr["nonzero_memory"][m] = nr["alloc_memory"][m] - 64 * synth.MiB
        # capacities above 2^47 (the int64 path) with part of them in use, and the N100_PRODUCT rows
        for k in np.nonzero(i % 5 == 4)[0]:
            cap = LA_CAPS[(k // 5) % len(LA_CAPS)]
            nr["alloc_milli_cpu"][k], nr["alloc_memory"][k] = cap, LA_CAPS[(k // 5 + 3) % len(LA_CAPS)]
            nr["nonzero_milli_cpu"][k] = cap // 3 if k % 2 else 0
            nr["nonzero_memory"][k] = (cap // 7) % int(nr["alloc_memory"][k])
        for k, (cap, nz, _) in zip(np.nonzero(i % 5 == 0)[0], _la_cases.N100_PRODUCT):
            nr["alloc_milli_cpu"][k] = nr["alloc_memory"][k] = cap
            nr["nonzero_milli_cpu"][k] = nr["nonzero_memory"][k] = nz
    return nr


def tombstones(n, pct, seed):
    """The rows deleted again. 90 %: in a table of three tiles the middle tile
    holds no present row, and every present row of the last tile is unschedulable
    (no feasible row there for a pod without the toleration)."""
    if pct == 0:
        return np.zeros(0, dtype=np.int64)
    u = synth.stream_u64(seed, 77, 0, n) % np.uint64(100)
    dead = u < np.uint64(pct)
    if n > 2 * T:
        dead[T:2 * T] = True
        dead[2 * T + 1] = False
    return np.nonzero(dead)[0]


def case(ps, nodes, pods, node_base=0, dead=(), weights=(1, 1), seed=1, term_sets=None, req_sets=None,
         max_nodes=None, tag=""):
    c = dict(plugin_set=ps, nodes=nodes, pods=pods, node_base=node_base, dead=np.asarray(dead, dtype=np.int64),
             weights=weights, seed=seed, max_nodes=max_nodes or len(nodes), tag=tag)
    if ps == 4:
        c["term_sets"] = synth.nam_term_sets_ext(N_SETS, seed=seed) if term_sets is None else term_sets
        c["req_sets"] = synth.nam_required_sets(N_SETS, seed=seed) if req_sets is None else req_sets
    return c


def family(ps):
    """The family's cases of one plugin set."""
    out = []
    for si, n in enumerate(SIZES):
        for pct in TOMBSTONES:
            for base in NODE_BASES:
                seed = 100 + 10 * si + (1 if pct else 0) + (4 if base else 0)
                nr = base_nodes(ps, n, seed)
                dead = tombstones(n, pct, seed)
                if pct and n > 2 * T:
                    nr["unschedulable"][2 * T:] = 1
                out.append(case(ps, nr, base_pods(ps, seed), node_base=base, dead=dead,
                                weights=(3, 2) if base else (1, 1), seed=seed, tag=f"set{ps} n={n} dead={pct}% base={base}"))
    return out


def tt_f_case(F):
    """MS_PLUGINS_NU_TT_NN with exactly F feasible rows for the pods that tolerate no
    hard taint, spread over three tiles; a pod tolerating every hard taint sees
    them all (F straddling the tiles). PreferNoSchedule counts run through 0..8;
    row 7 carries a second hard taint no pod but the last tolerates."""
    n = 2 * T + 37
    nr = synth.nodes(n, seed=40 + F)
    nr["unschedulable"] = 0
    i = np.arange(n)
    nr["taints"] = 1 | ((((1 << (i % 9)) - 1) & 0xFF) << 8)
    spots = [5, T - 1, T, 2 * T + 3, 2 * T + 36][:F]
    nr["taints"][spots] &= ~np.uint32(1)
    nr["taints"][7] |= 2
    pr = base_pods(3, 40 + F)
    synth.set_tolerations(pr, np.zeros(N_PODS, dtype=np.uint32), pr["pref_weight"].astype(np.uint32))
    pr["pref_zone"][30:36] = 1        # tolerates hard id 0: every row but 7 is feasible
    pr["pref_weight"][30:33] = 0      # ... and no soft taint: all nine raw counts score
    pr["pref_zone"][39] = 0xFF
    return case(3, nr, pr, node_base=33_333, seed=40 + F, tag=f"tt F={F}")


def tt_one_zero_case():
    """Raw counts [1, 0]: the in-loop hook gives [100, 100] (a two-pass normalise [0, 100])."""
    nr = synth.nodes(2, seed=9)
    nr["unschedulable"] = 0
    nr["taints"] = [1 << 8, 0]
    pr = base_pods(3, 9)
    pr["pref_zone"] = pr["pref_weight"] = 0
    return case(3, nr, pr, seed=9, tag="tt [1, 0]")


def tt_counts_case():
    """65 rows whose raw counts cycle 0..8, pods tolerating nothing soft."""
    nr = synth.nodes(65, seed=10)
    nr["taints"] = (((1 << (np.arange(65) % 9)) - 1) & 0xFF) << 8
    pr = base_pods(3, 10)
    pr["pref_zone"] = pr["pref_weight"] = 0
    return case(3, nr, pr, seed=10, tag="tt counts 0..8")


def nam_kat_case(filtered):
    """raw [30, 120, 250] -> [33, 40, 100]; the middle node filtered by a required set: [40, 100]."""
    nr, pr, ts, rq = _nam_required_cases.inloop_cluster()
    if not filtered:
        rq = np.zeros((0, _lib.NAM_REQ_SET_BYTES), dtype=np.uint8)
    return case(4, nr, pr, weights=(7, 1), seed=5, term_sets=ts, req_sets=rq, tag=f"nam KAT filtered={filtered}")


def nam_late_case():
    """Three tiles of raw 30 rows (zone 1), some 120s (zone 2), ONE raw 250 node in
    the last tile: it rescales every earlier row, whatever window is asked for; a
    run of raw 101 rows (zone 4) walks 100 -> 99 -> 98 ... in the middle tile."""
    n = 2 * T + 37
    nr = synth.nodes(n, seed=21)
    nr["zone"] = 1
    nr["zone"][np.arange(n) % 37 == 5] = 2
    nr["zone"][T + 10:T + 50] = 4
    nr["zone"][2 * T + 20] = 3
    nr["zone"][:3] = 0  # raw 0 before the anchor
    pr = base_pods(4, 21)
    pr["pref_zone"], pr["pref_weight"] = 1, 0
    pr["pref_zone"][30:] = 2
    ts = _lib.nam_term_sets_ext_array([KAT_TERMS + [], [(30, 0b01110, FULL), (90, 0b01100, FULL), (100, 0b11000, FULL),
                                                         (1, 0b10000, FULL)]])
    rq = np.zeros((0, _lib.NAM_REQ_SET_BYTES), dtype=np.uint8)
    return case(4, nr, pr, node_base=33_333, weights=(3, 2), seed=21, term_sets=ts, req_sets=rq, tag="nam late rescale")


def nam_r101_case():
    """T + 1 rows, all raw 101 but a few raw 30s: 200 rescales by 101 in a row."""
    n = T + 1
    nr = synth.nodes(n, seed=22)
    nr["zone"] = 4
    nr["zone"][::50] = 1
    pr = base_pods(4, 22)
    pr["pref_zone"], pr["pref_weight"] = 1, 0
    ts = _lib.nam_term_sets_ext_array([[(30, 0b00010, FULL)] + R101_TERMS])
    rq = np.zeros((0, _lib.NAM_REQ_SET_BYTES), dtype=np.uint8)
    return case(4, nr, pr, seed=22, term_sets=ts, req_sets=rq, tag="nam x101")


def na_anchor_case():
    """MS_PLUGINS_NU_NN_NA, three tiles: zone 3 first at row T + 7 (the anchor of
    the pods preferring it), zone 5 only at row 2 T + 30, weights (3, 2)."""
    n = 2 * T + 37
    nr = synth.nodes(n, seed=23, zones=True)
    nr["zone"][nr["zone"] == 3] = 1
    nr["zone"][nr["zone"] == 5] = 2
    nr["zone"][[T + 7, T + 90, 2 * T + 2]] = 3
    nr["zone"][2 * T + 30] = 5
    nr["unschedulable"][[T + 7, 2 * T + 30]] = 0
    pr = base_pods(2, 23)
    pr["pref_zone"][:20], pr["pref_weight"][:20] = 3, 60
    pr["pref_zone"][20:30], pr["pref_weight"][20:30] = 5, 100
    return case(2, nr, pr, node_base=33_333, weights=(3, 2), seed=23, tag="na anchor")


def la_case():
    """Every LA capacity against every pod, on 130 rows."""
    return case(1, base_nodes(1, 130, 31), base_pods(1, 31), node_base=0, seed=31, tag="la pairs")


def directed():
    return ([tt_f_case(F) for F in range(6)] + [tt_one_zero_case(), tt_counts_case(), nam_kat_case(False),
            nam_kat_case(True), nam_late_case(), nam_r101_case(), na_anchor_case(), la_case()])


_CACHE = {}


def reference(c):
    """The case's reference (rows, summaries), computed once per session."""
    import _explain_ref

    k = id(c)
    if k not in _CACHE:
        _CACHE[k] = (c, _explain_ref.explain(c))
    return _CACHE[k][1]


_ALL = {}


def all_cases():
    """Every case, built once: {tag: case}."""
    if not _ALL:
        for ps in range(5):
            for c in family(ps):
                _ALL[c["tag"]] = c
        for c in directed():
            _ALL[c["tag"]] = c
    return _ALL
