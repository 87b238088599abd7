"""Single (pod, node) pairs of MS_PLUGINS_NU_NRF_NN_LA made observable through
the ordinary ABI, with their exact model in Python integers.

NodeResourcesFit reads Requested, LeastAllocated reads NonZeroRequested, both
read Allocatable. In a table of M rows, row i's free amounts are made
(i, M - i) by Requested = Allocatable - (i, M - i), and pod i requests exactly
(i, M - i): it fits row i and no other (j <= i and M - j <= M - i). Allocatable
and both NonZeroRequested columns are then free to carry the probed triple
(cap, nz, n), and the pod's score (or the score field of its key) is
NodeNumber + (s_cpu + s_mem) / 2 of exactly that pair. Mirrored probes (CPU
triple == memory triple) make the halving lossless; crossed ones (independent
triples) catch swapped columns.

Tested domain (stated, checked by check_domain): 0 <= cap <= 2^56 so that
100 * (cap - nz - n) stays inside int64 (above it the reference's own product
wraps and the C oracle's is undefined), nz >= 0, 0 <= n < 2^62. Against a
capacity below 2^53, pods with n >= 2^53 / 2^55 (the engine's kPfOk and n100
clamps) appear only where n > cap: their expected score is 0.

Which evaluation of the pair a kernel takes is chosen per wave or per tile
from the data (ms_rows.h, ms_seq.hip), tiles being 64..256 rows starting at a
multiple of 16, pod chunks 8 or 16 pods starting at a multiple of 8. The table
kinds steer that choice:
  fast       every capacity < 2^41, every pod request < 2^53 (but the few
             clamp pods, together in the last table): the binary64 forms
  general    an unschedulable decoy row of capacity 2^41 at every row that is a
             multiple of 16: every tile and wave carries a row outside the
             binary64 range, so all probes take the f32 + int64 form; adds
             probe capacities in [2^41, 2^53)
  huge       decoys of capacity 2^53: the form compiled with the huge-row
             branch evaluates the ordinary rows too; adds probes in [2^53, 2^56]
  slowpods   the fast rows, with an unplaceable decoy pod of non-zero request
             2^53 at every pod index that is a multiple of 8
Test infrastructure, never product code.
"""
from __future__ import annotations

import numpy as np

import _pyref

KINDS = ("fast", "general", "huge", "slowpods")
K_FAST_CAP = 1 << 41   # ms_rows.h kFastCap
K_HUGE_CAP = 1 << 53   # ms_rows.h kHugeCap (and kFastReq, the pods' binary64 limit)
CAP_MAX = 1 << 56
N_MAX = 1 << 62
MIB = 1 << 20
ROWS_PER_DECOY = 16
PODS_PER_DECOY = 8
PROBES_PER_TABLE = 1000  # not a multiple of 16 or 64: the last tile and wave are short
ALLOWED_PODS = 110
SEED = 0x5EED_0123_4567

CODE_SUCCESS, CODE_UNSCHEDULABLE = 0, 2
MASK_NU, MASK_NRF = 1, 2

# capacities below 2^41: tiny ones, millicore counts, primes, MiB multiples, the f32
# integer limit, the lo/hi split of the int64 correction, the last fast capacity
FAST_CAPS = (
    1, 3, 99, 100, 101,
    250, 300, 500, 750, 1000, 1900, 3920, 7910, 64000, 192000,
    7, 97, 257, 65537, 999983, (1 << 31) - 1,
    MIB, 3 * MIB, 512 * MIB, 7919 * MIB, 16384 * MIB, 257251 * MIB, 1536 * 1024 * MIB,
    (1 << 24) - 1, 1 << 24, (1 << 24) + 1,
    (1 << 32) - 1, 1 << 32, (1 << 32) + 1,
    K_FAST_CAP - 1,
)
GENERAL_CAPS = (K_FAST_CAP, K_FAST_CAP + 1, 1 << 45, 3 * (1 << 44) + 12345, 5 * 1024 * 1024 * MIB,
                (1 << 47) + 1, 3 * (1 << 50) + 7, (1 << 52) + 1, K_HUGE_CAP - 2, K_HUGE_CAP - 1)
HUGE_CAPS = (K_HUGE_CAP, K_HUGE_CAP + 1, (1 << 55) + 12347, CAP_MAX - 1, CAP_MAX)
# pod requests at and past the clamps, against these capacities (all below 2^53: score 0)
CLAMP_REQUESTS = (K_HUGE_CAP, K_HUGE_CAP + 1, 1 << 55, (1 << 55) + 3, N_MAX - 1)
CLAMP_CAPS = (1000, 16384 * MIB, K_FAST_CAP - 1)
# Named regression triples (cap, nz, n).
# N100_PRODUCT: load_pod's 100 * min(n, 2^55) went through binary64 (min(long, long long)
# picks the mixed-type overload), so 100 n was rounded to 53 bits once n > 2^53 / 100 and
# the general form's correction compare 100 d < m * cap flipped next to a step: 9 for 8,
# 9 for 10, 37 for 36, 35 for 34, 20 for 19 on the first five (the sixth: the fifth with
# part of the request already on the node).
N100_PRODUCT = (
    ((1 << 53) - 1, 0, 8196551321814302),
    ((1 << 53) - 2, 0, 8106479329266891),
    ((1 << 53) - 2, 0, 5674535530486824),
    ((1 << 53) - 1000, 0, 5854679515580995),
    ((1 << 53) - 1000, 0, 7205759403791994),
    ((1 << 53) - 1000, 2000000000000000, 5205759403791994),
)
REGRESSIONS = {"n100_product": N100_PRODUCT}
# steps whose both sides the crossed probes take
CROSS_STEPS = (1, 33, 50, 67, 100)


# ---- the model (Python integers) ---------------------------------------------
def la_score(cap, nz, n):
    """leastRequestedScore of one resource: requested = nz + n."""
    cap, nz, n = int(cap), int(nz), int(n)
    return 0 if cap == 0 or nz + n > cap else (cap - nz - n) * 100 // cap


def pair_score(tc, tm, nn):
    """NodeNumber + LeastAllocated of a pair: tc / tm the CPU / memory (cap, nz, n)."""
    return nn + (la_score(*tc) + la_score(*tm)) // 2


def nn_score(pod_digit, node_digit):
    return 10 if node_digit != 0xFF and int(pod_digit) == int(node_digit) else 0


def fits(node, pod):
    """NodeResourcesFit.fitsRequest on one node record and one pod record."""
    bad = int(node["pod_count"]) + 1 > int(node["allowed_pods"])
    rc, rm = int(pod["req_milli_cpu"]), int(pod["req_memory"])
    if rc == 0 and rm == 0:
        return not bad
    bad = bad or rc > int(node["alloc_milli_cpu"]) - int(node["req_milli_cpu"])
    bad = bad or rm > int(node["alloc_memory"]) - int(node["req_memory"])
    return not bad


def filter_pair(node, pod):
    """(feasible, mask of the FIRST failing filter plugin) of one present node."""
    if node["unschedulable"] and not pod["tolerates_unschedulable"]:
        return False, MASK_NU
    if not fits(node, pod):
        return False, MASK_NRF
    return True, 0


def key_of(score, seed, pod_ordinal, node):
    return _pyref.key(int(score), _pyref.h32(seed, int(pod_ordinal), int(node)), int(node))


# ---- probes ----------------------------------------------------------------------
def step_points(cap, steps=range(1, 101)):
    """d = cap - nz - n on both sides of every k * cap / 100 step: ceil(k cap / 100)
    and that value -2, -1, +1, +2; with d = 0, -1 and cap (d <= cap as nz, n >= 0)."""
    ds = {0, -1, cap}
    for k in steps:
        b = -((-k * cap) // 100)
        ds.update(b + e for e in (-2, -1, 0, 1, 2))
    return sorted(d for d in ds if -2 <= d <= cap)


def triples(cap, steps=range(1, 101)):
    """(cap, nz, n) for every step point with nz = 0, nz = a mid value and n = 0,
    and over-committed nodes (nz > cap: score 0)."""
    out = []
    mid = cap // 3
    for d in step_points(cap, steps):
        out.append((cap, 0, cap - d))
        if mid and cap - mid - d >= 0:
            out.append((cap, mid, cap - mid - d))
        out.append((cap, cap - d, 0))
    over = cap + 1 + cap // 7
    out += [(cap, over, 0), (cap, over, 1), (cap, over, cap)]
    return list(dict.fromkeys(out))


def probes(kind):
    """The (CPU triple, memory triple) list of a table kind: mirrored probes of
    every capacity, then crossed ones, then the clamp pods."""
    caps = list(FAST_CAPS)
    if kind == "general":
        caps += GENERAL_CAPS
    if kind == "huge":
        caps += HUGE_CAPS
    out = []
    for cap in caps:
        out += [(t, t) for t in triples(cap)]
    for a, b in zip(caps, caps[1:] + caps[:1]):
        ta, tb = triples(a, CROSS_STEPS), triples(b, CROSS_STEPS)
        out += [(ta[i % len(ta)], tb[(3 * i + 1) % len(tb)]) for i in range(max(len(ta), len(tb)))]
    for cap in CLAMP_CAPS:
        out += [((cap, 0, n), (cap, 0, n)) for n in CLAMP_REQUESTS]
    return out


def check_domain(probe_list):
    for tc, tm in probe_list:
        for cap, nz, n in (tc, tm):
            assert 0 <= cap <= CAP_MAX and nz >= 0 and 0 <= n < N_MAX, (cap, nz, n)
            # past the pods' binary64 limit: a clamp pod (score 0) or the request of a huge row
            assert n < K_HUGE_CAP or cap < n or cap >= K_HUGE_CAP, (cap, nz, n)


# ---- tables ----------------------------------------------------------------------
class Table:
    """One table of a kind: node records, pod records and the model's outputs.
    probe_row[k] / probe_pod[k]: the row and the pod of this table's k-th probe."""


def _node_digit(r):
    return 0xFF if r % 11 == 10 else r % 10


def _pod_digit(r):
    return r % 10 if r % 2 == 0 else (r + 3) % 10


def build_table(kind, chunk, node_rec, pod_rec, seed=SEED, ordinal0=0):
    """The table of `chunk` (a list of probes) in form `kind`."""
    assert kind in KINDS
    decoy_cap = {"general": K_FAST_CAP, "huge": K_HUGE_CAP}.get(kind)
    n_probe = len(chunk)
    if decoy_cap:  # rows 0, 16, 32, .. are decoys
        n_rows = n_probe + -(-n_probe // (ROWS_PER_DECOY - 1))
        probe_row = [r for r in range(n_rows) if r % ROWS_PER_DECOY][:n_probe]
        n_rows = probe_row[-1] + 1
    else:
        n_rows, probe_row = n_probe, list(range(n_probe))
    M = n_rows
    nodes = np.zeros(M, dtype=node_rec)
    nodes["allowed_pods"] = ALLOWED_PODS
    nodes["pod_count"] = np.arange(M) % 50
    nodes["name_digit"] = [_node_digit(r) for r in range(M)]
    if decoy_cap:
        dec = np.arange(0, M, ROWS_PER_DECOY)
        nodes["unschedulable"][dec] = 1
        nodes["alloc_milli_cpu"][dec] = decoy_cap
        nodes["alloc_memory"][dec] = decoy_cap
    rows = np.array(probe_row)
    c = np.array([tc for tc, _ in chunk], dtype=np.int64)  # columns: cap, nz, n
    m = np.array([tm for _, tm in chunk], dtype=np.int64)
    nodes["alloc_milli_cpu"][rows], nodes["nonzero_milli_cpu"][rows] = c[:, 0], c[:, 1]
    nodes["alloc_memory"][rows], nodes["nonzero_memory"][rows] = m[:, 0], m[:, 1]
    nodes["req_milli_cpu"][rows] = c[:, 0] - rows
    nodes["req_memory"][rows] = m[:, 0] - (M - rows)
    # pods: probe k -> pod index probe_pod[k]
    if kind == "slowpods":  # pods 0, 8, 16, .. are decoys
        n_pods = n_probe + -(-n_probe // (PODS_PER_DECOY - 1))
        probe_pod = [p for p in range(n_pods) if p % PODS_PER_DECOY][:n_probe]
        n_pods = probe_pod[-1] + 1
    else:
        n_pods, probe_pod = n_probe, list(range(n_probe))
    pods = np.zeros(n_pods, dtype=pod_rec)
    pods["ordinal"] = ordinal0 + np.arange(n_pods)
    pods["name_digit"] = 0
    pods["req_milli_cpu"] = M + 1  # decoys: fit nowhere (free CPU < M)
    pods["req_memory"] = M + 1
    pods["nonzero_milli_cpu"] = K_HUGE_CAP
    pods["nonzero_memory"] = K_HUGE_CAP
    t = Table()
    t.kind, t.M, t.nodes, t.pods, t.chunk, t.seed = kind, M, nodes, pods, chunk, seed
    t.probe_row, t.probe_pod = np.array(probe_row), np.array(probe_pod)
    t.node = np.full(n_pods, -1, np.int32)
    t.code = np.full(n_pods, CODE_UNSCHEDULABLE, np.int32)
    t.score = np.zeros(n_pods, np.int64)
    any_nu = bool(decoy_cap)
    t.mask = np.full(n_pods, MASK_NRF | (MASK_NU if any_nu else 0), np.uint32)
    t.key = np.zeros(n_pods, np.uint64)
    # filter flags of the sweeps: byte 0 some node NU-rejected, byte 1 some node NRF-rejected
    # (every pod is rejected by every probe row but its own)
    t.flags = np.full(n_pods, (0x100 if n_probe > 1 else 0) | (1 if any_nu else 0), np.uint32)
    if kind == "slowpods":
        t.flags[::PODS_PER_DECOY] |= 0x100
    pp = t.probe_pod
    pods["req_milli_cpu"][pp], pods["req_memory"][pp] = rows, M - rows
    pods["nonzero_milli_cpu"][pp], pods["nonzero_memory"][pp] = c[:, 2], m[:, 2]
    pods["name_digit"][pp] = [_pod_digit(r) for r in probe_row]
    scores = [pair_score(tc, tm, nn_score(_pod_digit(r), _node_digit(r))) for (tc, tm), r in zip(chunk, probe_row)]
    t.node[pp], t.code[pp], t.score[pp], t.mask[pp] = rows, CODE_SUCCESS, scores, 0
    t.key[pp] = np.array([key_of(s, seed, ordinal0 + p, r) for s, p, r in zip(scores, probe_pod, probe_row)],
                         dtype=np.uint64)
    return t


def after_binds(t):
    """The node records after every probe pod was bound to its row (NodeInfo.AddPod)."""
    a = t.nodes.copy()
    r, p = t.probe_row, t.probe_pod
    a["pod_count"][r] += 1
    for f_n, f_p in (("req_milli_cpu", "req_milli_cpu"), ("req_memory", "req_memory"),
                     ("nonzero_milli_cpu", "nonzero_milli_cpu"), ("nonzero_memory", "nonzero_memory")):
        a[f_n][r] += t.pods[f_p][p]
    return a


_CACHE = {}


def tables(kind, node_rec, pod_rec):
    """Every table of a kind (built once per session, never modified): the kind's
    probes in chunks of PROBES_PER_TABLE, the last chunk filled up from the front so
    that all tables of a kind have the same shape (one engine serves them all)."""
    if kind not in _CACHE:
        pl = probes(kind)
        check_domain(pl)
        P = PROBES_PER_TABLE
        pad = -len(pl) % P
        full = pl + pl[:pad]
        _CACHE[kind] = (len(pl), [build_table(kind, full[a:a + P], node_rec, pod_rec, ordinal0=7 * a)
                                  for a in range(0, len(full), P)])
    return _CACHE[kind]


def describe(t, p):
    """The probe behind pod p of table t (for assertion messages)."""
    k = int(np.nonzero(t.probe_pod == p)[0][0]) if p in t.probe_pod else None
    if k is None:
        return f"{t.kind} decoy pod {p}"
    tc, tm = t.chunk[k]
    return f"{t.kind} row {int(t.probe_row[k])} pod {p}: cpu (cap, nz, n) = {tc}, mem = {tm}, model score {int(t.score[p])}"


# ---- the validator walk ----------------------------------------------------------
WALK_CAPS = (100, 3920, 999983, (1 << 24) + 1, 16384 * MIB, (1 << 32) + 1, K_FAST_CAP - 1,
             K_FAST_CAP, 3 * (1 << 44) + 12345, K_HUGE_CAP - 1,
             K_HUGE_CAP, (1 << 55) + 12347, CAP_MAX)


def walk(cap, pod_rec, node_digit, ordinal0=0):
    """Pods for ONE node of capacity `cap` (both resources), NonZeroRequested 0 at
    the start: zero Fit requests, non-zero requests = the successive differences of
    the descending step points, so every bind moves the node to the next probe
    point; the last pod over-commits it (d = -1). Returns (pods, scores, final nz)."""
    ds = [d for d in reversed(step_points(cap)) if d >= -1]
    pods = np.zeros(len(ds), dtype=pod_rec)
    pods["ordinal"] = ordinal0 + np.arange(len(ds))
    scores, nz = [], 0
    for j, d in enumerate(ds):
        n = cap - nz - d
        assert 0 <= n < N_MAX and (j == 0 or n > 0)
        pods["nonzero_milli_cpu"][j] = pods["nonzero_memory"][j] = n
        pods["name_digit"][j] = j % 10
        scores.append(pair_score((cap, nz, n), (cap, nz, n), nn_score(j % 10, node_digit)))
        nz += n
    return pods, np.array(scores, np.int64), nz
