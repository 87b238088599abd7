"""Reference of Engine.explain (DESIGN.md §2 "Explain"), built from the flat
records and independent of the device code. Test infrastructure.

Per pod, over the table in LIST order:
  filters   restated here in plugin order, the first failure wins
            (minisched.go:130-137): NodeUnschedulable; NodeResourcesFit
            (_la_cases.fits' rule, vectorised); TaintToleration's hard taints;
            NodeAffinity's required terms (_nam_required_ref.passes_rows on the
            decoded id sets);
  raw       plain Python / numpy integers: NodeNumber 10 or 0, LeastAllocated by
            _la_cases.la_score (Python big integers), the preferred-term weight
            sums, the count of untolerated PreferNoSchedule taints;
  final     the oracle's LITERAL in-loop hook on the pod's feasible list
            (_oracle.tt_inloop / nam_inloop with literal=True; the identity for
            plugins without ScoreExtensions), times the plugin weight;
  key       rule r3. Computed in numpy for speed (_nam_required_ref.keys_r3);
            tests/test_explain_ref.py checks that form against the oracle's
            msor_h32 / msor_key pair by pair.
A case is a dict: plugin_set, node_base, max_nodes, nodes (records of ordinals
node_base + arange(len)), dead (row indices deleted again), pods, weights, seed,
and for set 4 term_sets (n, 272) and req_sets (n, 260).
"""
from __future__ import annotations

import numpy as np

import _la_cases
import _nam_required_ref as nref
import _oracle
from minisched_amd import _lib

ABSENT = _lib.EXPLAIN_ABSENT


def node_state(case):
    """(present mask, node records) over the context's max_nodes rows."""
    n = case["max_nodes"]
    nodes = np.zeros(n, dtype=_lib.NODE_REC)
    nodes["name_digit"] = 0xFF
    k = len(case["nodes"])
    nodes[:k] = case["nodes"]
    present = np.zeros(n, dtype=bool)
    present[:k] = True
    present[np.asarray(case.get("dead", ()), dtype=np.int64)] = False
    return present, nodes


def _fits(nodes, pod):
    bad = nodes["pod_count"].astype(np.int64) + 1 > nodes["allowed_pods"].astype(np.int64)
    rc, rm = int(pod["req_milli_cpu"]), int(pod["req_memory"])
    if rc == 0 and rm == 0:
        return ~bad
    bad = bad | (rc > nodes["alloc_milli_cpu"] - nodes["req_milli_cpu"])
    bad = bad | (rm > nodes["alloc_memory"] - nodes["req_memory"])
    return ~bad


def _popcount8(x):
    x = np.asarray(x, dtype=np.int64)
    return sum((x >> b) & 1 for b in range(8))


def explain(case):
    """(rows[n_pods, max_nodes], summaries[n_pods]) as Engine.explain returns them
    for the whole node range of the context."""
    ps = case["plugin_set"]
    present, nodes = node_state(case)
    pods = case["pods"]
    n = len(nodes)
    w_nn, w_na = (int(w) or 1 for w in case.get("weights", (1, 1))) if ps in (2, 4) else (1, 1)
    rows = np.zeros((len(pods), n), dtype=_lib.EXPLAIN_ROW)
    sums = np.zeros(len(pods), dtype=_lib.EXPLAIN_SUMMARY)
    unsched = nodes["unschedulable"] != 0
    digit = nodes["name_digit"].astype(np.int64)
    ordinals = case["node_base"] + np.arange(n, dtype=np.int64)
    if ps == 4:
        pref = nref.decode_preferred(case["term_sets"])
        req = nref.decode_required(case["req_sets"])
        n_ids = max(len(pref), len(req))
        zl = list(zip(nodes["zone"].tolist(), nodes["label2"].tolist()))
    for j, pod in enumerate(pods):
        status = np.full(n, ABSENT, dtype=np.int64)
        status[present] = 0
        status[present & unsched & (pod["tolerates_unschedulable"] == 0)] = 1
        rest = status == 0
        raw1 = np.zeros(n, dtype=np.int64)
        if ps == 1:
            status[rest & ~_fits(nodes, pod)] = 2
            for i in np.nonzero(status == 0)[0]:
                x = nodes[i]
                raw1[i] = (_la_cases.la_score(x["alloc_milli_cpu"], x["nonzero_milli_cpu"], pod["nonzero_milli_cpu"]) +
                           _la_cases.la_score(x["alloc_memory"], x["nonzero_memory"], pod["nonzero_memory"])) // 2
        elif ps == 2:
            if pod["pref_zone"] != 0:
                raw1 = np.where(nodes["zone"] == pod["pref_zone"], int(pod["pref_weight"]), 0).astype(np.int64)
        elif ps == 3:
            tn = nodes["taints"].astype(np.int64)
            status[rest & ((tn & 0xFF & ~int(pod["pref_zone"])) != 0)] = 4
            raw1 = _popcount8((tn >> 8) & 0xFF & ~int(pod["pref_weight"]))
        elif ps == 4:
            sid = int(pod["pref_zone"]) | int(pod["pref_weight"]) << 8
            if sid > n_ids:
                sid = 0
            status[rest & ~nref.passes_rows(nref.required_of(sid, req), nodes)] = 8
            pset = pref[sid - 1] if 1 <= sid <= len(pref) else []
            memo = {}
            for i, (z, l) in enumerate(zl):
                if (z, l) not in memo:
                    memo[(z, l)] = sum(w for w, zm, lm in pset if w and (zm >> z) & 1 and (lm >> l) & 1)
                raw1[i] = memo[(z, l)]
        feas = np.nonzero(status == 0)[0]
        rows["status"][j] = status
        s = sums[j]
        s["present"], s["feasible"] = int(present.sum()), len(feas)
        for b in range(4):
            s["rejected"][b] = int((status == 1 << b).sum())
        if len(feas) == 0 or pod["name_digit"] < 0:
            continue  # nothing is scored: FitError, or NodeNumber.Score fails on the first node
        raw0 = np.where((digit[feas] <= 9) & (digit[feas] == int(pod["name_digit"])), 10, 0)
        r1 = raw1[feas]
        if ps in (2, 4):
            fin = _oracle.nam_inloop(r1, literal=True)
        elif ps == 3:
            fin = _oracle.tt_inloop(r1, literal=True)
        else:
            fin = r1  # no ScoreExtensions: the hook is the identity (nodenumber.go:98-100)
        w0, w1 = raw0 * w_nn, fin * w_na
        keys = nref.keys_r3(case["seed"], pod["ordinal"], ordinals[feas], w0 + w1)
        rows["key"][j, feas] = keys
        rows["raw"][j, feas, 0], rows["raw"][j, feas, 1] = raw0, r1
        rows["weighted"][j, feas, 0], rows["weighted"][j, feas, 1] = w0, w1
        s["best_key"] = keys.max()
    return rows, sums


def decode(summary):
    """(node, score, code, mask) of a pod from its summary, as ms_result holds them.
    A pod with feasible nodes and no key is the non-digit pod's score error."""
    k = int(summary["best_key"])
    if int(summary["feasible"]) == 0:
        mask = sum(1 << b for b in range(4) if int(summary["rejected"][b]))
        return -1, 0, 2, mask
    if k == 0:
        return -1, 0, 1, 0
    return 0xFFFFF - (k & 0xFFFFF), k >> 52, 0, 0


def same(got_rows, got_sums, want_rows, want_sums, tag):
    """Element for element on status, raw, weighted, key and every summary field."""
    for f in ("status", "raw", "weighted", "key", "_pad"):
        a, b = got_rows[f], want_rows[f]
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)[:6]
            raise AssertionError(f"{tag}: rows[{f}] differ at {bad.tolist()}: got "
                                 f"{[a[tuple(i)].tolist() for i in bad]} want {[b[tuple(i)].tolist() for i in bad]}")
    if got_sums is None:
        return
    for f in ("present", "feasible", "rejected", "best_key"):
        a, b = got_sums[f], want_sums[f]
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)[:6]
            raise AssertionError(f"{tag}: summaries[{f}] differ at {bad.tolist()}: got "
                                 f"{[a[tuple(i)].tolist() for i in bad]} want {[b[tuple(i)].tolist() for i in bad]}")
