"""NodeAffinity as a filter in MS_PLUGINS_NU_NN_NAM: two references, built
independently, that must agree before either judges the GPU.

1. schedule_literal: a restatement in Python of the cycle on the flat records
   and the id masks. Per pod the nodes in LIST order through NodeUnschedulable,
   then NodeAffinity's Filter (nodeSelector folded into every required term; a
   node passes when one term holds both its value ids; the first failing plugin
   is the one recorded for the node), then over the feasible nodes
   RunScorePlugins' in-loop DefaultNormalizeScore hook as written (the whole
   list after every node), the weighted sum, and selectHost by the r3 key.
2. schedule_tombstone: for each required set, the C oracle's schedule_nam_ext on
   a copy of the table whose rows failing the requirement are dead
   (allowed_pods = -1) for that set's pods; only the FitError mask is recomputed
   here, in numpy, by the rule of the issue: NodeAffinity iff a present node
   passed NodeUnschedulable and failed NodeAffinity, NodeUnschedulable iff a
   present node failed it. Pod ordinals ride in the records, so the tie-breaks
   are the oracle's own.
Test infrastructure, never product code.
"""
from __future__ import annotations

import numpy as np

from minisched_amd import _lib

MASK_NU, MASK_NA = 1, 8
CODE_SUCCESS, CODE_ERROR, CODE_UNSCHEDULABLE = 0, 1, 2
_M32 = np.uint64(0xFFFFFFFF)


def _int_of(b):
    return int.from_bytes(bytes(b), "little")


def decode_required(req_sets):
    """ms_nam_required_set records (uint8 (n, 260)) -> per set None (no
    requirement) or its terms [(zone id set, label2 id set), ...] as ints."""
    a = np.asarray(req_sets, dtype=np.uint8).reshape(-1, _lib.NAM_REQ_SET_BYTES)
    out = []
    for row in a:
        n = int(row[256])
        out.append(None if n == 0 else [(_int_of(row[64 * k:64 * k + 32]), _int_of(row[64 * k + 32:64 * k + 64]))
                                        for k in range(n)])
    return out


def decode_preferred(term_sets_ext):
    """ms_nam_term_set_ext records (uint8 (n, 272)) -> per set [(weight, zone id
    set, label2 id set), ...]."""
    a = np.asarray(term_sets_ext, dtype=np.uint8).reshape(-1, _lib.NAM_SET_EXT_BYTES)
    return [[(int(row[68 * k + 64]), _int_of(row[68 * k:68 * k + 32]), _int_of(row[68 * k + 32:68 * k + 64]))
             for k in range(_lib.NAM_TERMS)] for row in a]


def set_id(pods):
    return pods["pref_zone"].astype(np.int64) | pods["pref_weight"].astype(np.int64) << 8


def required_of(sid, req):
    return req[sid - 1] if 1 <= sid <= len(req) else None


def passes(terms, zone, label2):
    """RequiredNodeAffinity.Match on one node's value ids (terms None: no requirement)."""
    if terms is None:
        return True
    return any((zm >> zone) & 1 and (lm >> label2) & 1 for zm, lm in terms)


def passes_rows(terms, nodes):
    """passes() for every node record, as a bool array."""
    if terms is None:
        return np.ones(len(nodes), dtype=bool)
    pair = {}
    out = np.zeros(len(nodes), dtype=bool)
    for i, (z, l) in enumerate(zip(nodes["zone"].tolist(), nodes["label2"].tolist())):
        if (z, l) not in pair:
            pair[(z, l)] = passes(terms, z, l)
        out[i] = pair[(z, l)]
    return out


def inloop(raw):
    """RunScorePlugins' hook for NodeAffinity (reverse=false): the plugin's list
    starts zero-filled; after each node's score lands, DefaultNormalizeScore runs
    over the WHOLE list (later entries still 0)."""
    na = np.zeros(len(raw), dtype=np.int64)
    for k, r in enumerate(raw):
        na[k] = r
        m = int(na.max())
        if m > 0:
            na = 100 * na // m
    return na


def _mix32(x):
    x = x & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0xC2B2AE35)) & _M32
    return x


def _fmix32(h):
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def keys_r3(seed, pod_ordinal, node_ordinals, scores):
    """Rule r3 (include/minisched_gpu.h): score << 52 | h32 << 20 | (0xFFFFF - node)."""
    a = np.uint64(_fmix32(((seed ^ (seed >> 32)) & 0xFFFFFFFF) ^ int(pod_ordinal)))
    o = np.asarray(node_ordinals, dtype=np.uint64)
    h = _mix32(a + o * np.uint64(0x9E3779))
    return (np.asarray(scores, dtype=np.uint64) << np.uint64(52)) | (h << np.uint64(20)) | (np.uint64(0xFFFFF) - o)


def _outs(n):
    return dict(node=np.full(n, -1, np.int32), score=np.zeros(n, np.int64), code=np.zeros(n, np.int32),
                mask=np.zeros(n, np.uint32))


def schedule_literal(nodes, pods, term_sets_ext, req_sets, weights=(1, 1), seed=1, node_base=0, dead=()):
    """Reference 1. The in-loop hook's list depends on the pod only through its
    set id and toleration, so it is computed once per such pair and reused."""
    pref, req = decode_preferred(term_sets_ext), decode_required(req_sets)
    w_nn, w_na = (int(w) or 1 for w in weights)
    gone = np.zeros(len(nodes), dtype=bool)
    gone[np.asarray(dead, dtype=np.int64)] = True
    absent = (gone | (nodes["allowed_pods"] < 0)).tolist()
    unsched = (nodes["unschedulable"] != 0).tolist()
    zone, label2 = nodes["zone"].tolist(), nodes["label2"].tolist()
    digit = nodes["name_digit"].astype(np.int64)
    o = _outs(len(pods))
    memo = {}
    for j, p in enumerate(pods):
        sid, tol = int(p["pref_zone"]) | int(p["pref_weight"]) << 8, bool(p["tolerates_unschedulable"])
        if (sid, tol) not in memo:
            terms = required_of(sid, req)
            pset = pref[sid - 1] if 1 <= sid <= len(pref) else []
            mask, feas, raw = 0, [], []
            for i in range(len(nodes)):  # RunFilterPlugins: per node, the first failing plugin
                if absent[i]:
                    continue
                if unsched[i] and not tol:
                    mask |= MASK_NU
                    continue
                if not passes(terms, zone[i], label2[i]):
                    mask |= MASK_NA
                    continue
                feas.append(i)
                raw.append(sum(w for w, zm, lm in pset if w and (zm >> zone[i]) & 1 and (lm >> label2[i]) & 1))
            memo[(sid, tol)] = (mask, np.asarray(feas, dtype=np.int64), inloop(raw))
        mask, feas, na = memo[(sid, tol)]
        if len(feas) == 0:
            o["code"][j], o["mask"][j] = CODE_UNSCHEDULABLE, mask
        elif p["name_digit"] < 0:  # NodeNumber.Score fails on the first feasible node
            o["code"][j] = CODE_ERROR
        else:
            nn = np.where(digit[feas] == int(p["name_digit"]), 10, 0)
            k = keys_r3(seed, p["ordinal"], node_base + feas, w_nn * nn + w_na * na)
            best = int(k.max())
            o["node"][j], o["score"][j] = 0xFFFFF - (best & 0xFFFFF), best >> 52
    return o


def schedule_tombstone(oracle, nodes, pods, term_sets_ext, req_sets, weights=(1, 1), seed=1, node_base=0, dead=(),
                       literal=None):
    """Reference 2."""
    req = decode_required(req_sets)
    nodes = nodes.copy()
    if len(dead):
        nodes["allowed_pods"][np.asarray(dead)] = -1
    literal = len(nodes) <= 3000 if literal is None else literal
    w = tuple(int(x) or 1 for x in weights)
    present = nodes["allowed_pods"] >= 0
    unsched = nodes["unschedulable"] != 0
    sid = set_id(pods)
    group = np.where((sid >= 1) & (sid <= len(req)), sid, 0)
    o = _outs(len(pods))
    for g in np.unique(group):
        idx = np.nonzero(group == g)[0]
        terms = required_of(int(g), req)
        ok = passes_rows(terms, nodes)
        tab = nodes.copy()
        tab["allowed_pods"][~ok] = -1
        r = oracle.schedule_nam_ext(tab, pods[idx], term_sets_ext, weights=w, literal=literal, seed=seed,
                                    node_base=node_base)
        for k in ("node", "score", "code"):
            o[k][idx] = r[k]
        tol = pods["tolerates_unschedulable"][idx] != 0
        nu = np.where(tol, False, bool((present & unsched).any()))
        na = np.where(tol, bool((present & ~ok).any()), bool((present & ~unsched & ~ok).any()))
        o["mask"][idx] = np.where(r["code"] == CODE_UNSCHEDULABLE, nu * MASK_NU + na * MASK_NA, 0)
    return o


def _field(x, k):
    # (engine results are ms_result records, references are dicts)
    return x["plugin_mask" if k == "mask" and isinstance(x, np.ndarray) else k]


def same(got, want, tag):
    """node, code, score and mask element for element."""
    for k in ("node", "code", "score", "mask"):
        a, b = np.asarray(_field(got, k)).astype(np.int64), np.asarray(_field(want, k)).astype(np.int64)
        if not np.array_equal(a, b):
            bad = np.nonzero(a != b)[0][:8]
            raise AssertionError(f"{tag} {k} differs at {bad.tolist()}: got {a[bad].tolist()} want {b[bad].tolist()}")
