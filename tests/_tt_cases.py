"""Biased clusters for MS_PLUGINS_NU_TT_NN and a Python model that labels each
winner, shared by tests/test_tt_cases.py (CPU: the model against the C oracle,
and how many pods win in each category) and tests/test_gpu_tt_classes.py.
Test infrastructure, never product code.

TaintToleration takes no score weight, so only winners are visible, and in
random clusters nearly every winner is a middle row with raw count 0. These
clusters move the winner around:
  - every row carries a random set of 0..8 PreferNoSchedule ids ORed with a
    per-cluster base set that every row carries;
  - a pod tolerates a thermometer mask (ids 0..k-1) with a few bits flipped, so
    the least untolerated count over its list ranges over 0..8;
  - few rows carry a digit name (none at all in one cluster of each size), so a
    winning class often has no NodeNumber match (W0);
  - in every other cluster each middle row carries one more soft id, 7, which no
    pod of that cluster tolerates, than the first six and the last four rows,
    whose soft ids are the base set alone: the explicit entries (feasible ranks
    0, 1, 2 and the last) win;
  - NoSchedule ids on 3 % of the rows (more in the small clusters) and pods
    tolerating each with probability 0.3 move the rank parity per pod.
A pod's list depends on it only through (tolerates_unschedulable, tol_hard,
tol_soft); a cluster's pods are a few dozen such patterns times the digits.
"""
from __future__ import annotations

import functools

import numpy as np

import _nam_required_ref as ref
from minisched_amd import _lib

SMALL_SIZES = (5, 6, 7, 9, 12, 20, 40)
LARGE_SIZES = (2100, 4100, 4200, 6500)  # 2, 3, 3 and 4 row segments of kTtSegRows = 2,048
SMALL_VARIANTS, LARGE_VARIANTS = 9, 5
SEED = 131


def _popcount(x):
    x = np.asarray(x, dtype=np.int64)
    return sum((x >> b) & 1 for b in range(8))


def cluster(n, variant):
    """(nodes, pods) of size n. variant 0: no digit rows; odd variants: the explicit
    entries are favoured; variant 4 of a large size and 7 of a small one: no digit
    rows and all eight soft ids in the base set (every count is 8 minus the
    tolerated ids, so mid(c, 0) occurs for every c); variant 8 of a small size:
    the same with digit rows (mid(c, 1) for every c)."""
    large = n > 100
    rng = np.random.default_rng(1000 * n + variant)
    full_base = variant == (4 if large else 7) or (not large and variant == 8)
    favoured = variant % 2 == 1 and not full_base
    nr = np.zeros(n, dtype=_lib.NODE_REC)
    nr["allowed_pods"] = 110
    p_digit = 0.0 if variant in (0, 4 if large else 7) else (0.005 if large else 0.5)
    nr["name_digit"] = np.where(rng.random(n) < p_digit, rng.integers(0, 10, n), 255)
    nr["unschedulable"] = rng.random(n) < (0.10 if large else 0.25)
    top = 7 if favoured else 8  # (favoured: id 7 is kept for the middle rows)
    base = 0xFF if full_base else int(rng.integers(0, 1 << top)) & int(rng.integers(0, 1 << top))
    dens = rng.random(n)[:, None] * 0.9
    soft = ((rng.random((n, top)) < dens) @ (1 << np.arange(top))) | base
    hard = (rng.random((n, 8)) < (0.03 if large else 0.06) / 2) @ (1 << np.arange(8))
    if favoured:
        soft |= 0x80
        edge = np.r_[0:min(6, n), max(0, n - 4):n]
        soft[edge] = base
    nr["taints"] = (hard | (soft << 8)).astype(np.uint32)

    # pods: patterns x digits
    n_pat = 36 if large else 27
    k = rng.integers(0, top + 1, n_pat)
    tol_soft = (1 << k) - 1
    for _ in range(2):
        flip = rng.random(n_pat) < 0.5
        tol_soft = np.where(flip, tol_soft ^ (1 << rng.integers(0, top, n_pat)), tol_soft)
    tol_soft[:3] = (0, (1 << top) - 1, base & ((1 << top) - 1))
    tol_hard = (rng.random((n_pat, 8)) < 0.3) @ (1 << np.arange(8))
    tol_uns = rng.random(n_pat) < 0.5
    per = 24 if large else 22
    P = n_pat * per
    pr = np.zeros(P, dtype=_lib.POD_REC)
    pr["ordinal"] = rng.permutation(P) + 7
    pat = np.repeat(np.arange(n_pat), per)
    dig = np.tile(np.r_[np.arange(10), np.arange(10), rng.integers(0, 10, per - 21), -1], n_pat)
    order = rng.permutation(P)
    pat, dig = pat[order], dig[order]
    pr["name_digit"], pr["tolerates_unschedulable"] = dig, tol_uns[pat]
    pr["pref_zone"], pr["pref_weight"] = tol_hard[pat], tol_soft[pat]  # (tol_hard, tol_soft: synth.set_tolerations)
    return nr, pr


def clusters(sizes=None):
    """(size, variant) of every cluster of the family."""
    out = [(n, v) for n in SMALL_SIZES for v in range(SMALL_VARIANTS)]
    out += [(n, v) for n in LARGE_SIZES for v in range(LARGE_VARIANTS)]
    return [c for c in out if sizes is None or c[0] in sizes]


# ---- the model -------------------------------------------------------------
def inloop(counts):
    """RunScorePlugins' in-loop hook for TaintToleration (DefaultNormalizeScore,
    reverse = true) as written: the list starts zero-filled; after each row's
    count lands the WHOLE list, later entries included, becomes 100 - 100 v // max
    (all 100 when the maximum is 0). Every step maps equal values to equal values,
    so the list is kept as groups of entries that hold one value (group 0: the
    entries not yet scored) and each step is carried out once per group."""
    F = len(counts)
    vals, gid = [0], np.zeros(F, dtype=np.int64)
    for k, c in enumerate(counts):
        c = int(c)
        g = vals.index(c, 1) if c in vals[1:] else len(vals)
        if g == len(vals):
            vals.append(c)
        gid[k] = g
        m = max(vals[1:] if k == F - 1 else vals)  # (after the last row no unscored entry is left)
        vals = [100 if m == 0 else 100 - 100 * v // m for v in vals]
    return np.asarray(vals, dtype=np.int64)[gid]


def schedule(nodes, pods, seed=SEED, node_base=0):
    """The cycle per pod: NodeUnschedulable then TaintToleration's filter (the
    first failing plugin is recorded), the literal loop on the feasible rows'
    untolerated PreferNoSchedule counts, NodeNumber + TaintToleration, and
    selectHost by the r3 key. Returns node, code, score, mask and per pod a
    category: None (no winner), ("small", F) for F <= 4, "first0" / "first1" /
    "first2" / "last" by the winner's feasible rank, else ("mid", count, match),
    and with it the winner's feasible rank and F."""
    n = len(pods)
    o = dict(node=np.full(n, -1, np.int32), score=np.zeros(n, np.int64), code=np.zeros(n, np.int32),
             mask=np.zeros(n, np.uint32), cat=[None] * n, rank=np.full(n, -1), F=np.zeros(n, np.int64))
    present = nodes["allowed_pods"] >= 0
    uns = nodes["unschedulable"] != 0
    hard, soft = nodes["taints"].astype(np.int64) & 0xFF, (nodes["taints"].astype(np.int64) >> 8) & 0xFF
    digit = nodes["name_digit"].astype(np.int64)
    memo = {}
    for j, p in enumerate(pods):
        key = (int(p["tolerates_unschedulable"]), int(p["pref_zone"]), int(p["pref_weight"]))
        if key not in memo:
            nu = present & uns & (key[0] == 0)
            tt = present & ~nu & ((hard & ~key[1]) != 0)
            feas = np.nonzero(present & ~nu & ~tt)[0]
            cnt = _popcount(soft[feas] & ~key[2])
            memo[key] = (feas, cnt, inloop(cnt), (1 if nu.any() else 0) | (4 if tt.any() else 0))
        feas, cnt, tts, mask = memo[key]
        F = len(feas)
        o["F"][j] = F
        if F == 0:
            o["code"][j], o["mask"][j] = 2, mask
        elif p["name_digit"] < 0:  # NodeNumber.Score fails on the first feasible node
            o["code"][j] = 1
        else:
            nn = np.where(digit[feas] == int(p["name_digit"]), 10, 0)
            keys = ref.keys_r3(seed, p["ordinal"], node_base + feas, nn + tts)
            k = int(keys.argmax())
            best = int(keys[k])
            o["node"][j], o["score"][j], o["rank"][j] = 0xFFFFF - (best & 0xFFFFF), best >> 52, k
            if F <= 4:
                o["cat"][j] = ("small", F)
            elif k < 3:
                o["cat"][j] = f"first{k}"
            elif k == F - 1:
                o["cat"][j] = "last"
            else:
                o["cat"][j] = ("mid", int(cnt[k]), int(nn[k] > 0))
    return o


@functools.lru_cache(maxsize=None)
def modelled(n, variant):
    nr, pr = cluster(n, variant)
    return schedule(nr, pr)


def tally(sizes):
    """{category: pods} over the clusters of the given sizes, and the pods that
    win with the rank-3 row of a five-row list."""
    cats, r3f5 = {}, 0
    for n, v in clusters(sizes):
        o = modelled(n, v)
        for c, k, F in zip(o["cat"], o["rank"], o["F"]):
            if c is not None:
                cats[c] = cats.get(c, 0) + 1
                r3f5 += int(F == 5 and k == 3)
    return cats, r3f5
