"""Inputs of the NodeAffinity-filter tests, shared by the CPU file (which checks
the references on them, and that they cover every FitError mask) and the GPU
file (which runs them). Test infrastructure."""
from __future__ import annotations

import numpy as np

from minisched_amd import synth

# (nodes, pods, sets, seed): the shapes of tests/test_gpu_nam.py, which hit the same
# edges: one node; a few; one row segment; 17 segments of 128 rows; several
# 1,024-row tiles' worth of segments (closed form above 3,000 nodes)
SHAPES = [(1, 40, 3, 1), (7, 200, 5, 2), (300, 500, 24, 3), (2100, 300, 40, 4), (9000, 400, 64, 5)]
WEIGHTS = [(2, 1), (7, 5)]
SHARD_CUTS = [(0, 4500, 9000), (0, 37, 38, 4000, 9000), (0, 3, 6000)]


def cluster(n_nodes, n_pods, n_sets, seed, n_req=None):
    """Node and pod records, preferred term sets (general form) and required
    sets (n_req of them, default one per preferred set)."""
    nr = synth.nodes(n_nodes, seed=seed, labels=True)
    pr = synth.pods(n_pods, seed=seed, term_sets=n_sets)
    pr["name_digit"][::23] = -1
    pr["tolerates_unschedulable"][::9] = 1
    nr["zone"][::17] = 255  # (id 255: a labelled node)
    nr["label2"][5::23] = 255
    n_req = n_sets if n_req is None else n_req
    return nr, pr, synth.nam_term_sets_ext(n_sets, seed=seed), synth.nam_required_sets(n_req, seed=seed)


def weights_case(weights):
    seed = 20 + weights[0]
    return cluster(5000, 600, 32, seed) + (np.arange(0, 5000, 7), seed)


def host_case():
    # (700 nodes: the literal loop is O(nodes^2) per pod class and the reference stays quick)
    return cluster(700, 2500, 16, 31) + (31,)


def shard_case(cuts):
    seed = 50 + len(cuts)
    n = cuts[-1]
    dead = np.arange(cuts[1], cuts[2]) if len(cuts) > 3 else np.arange(0, n, 13)
    return cluster(n, 1500, 48, seed) + (dead, seed)


def all_unschedulable_case():
    """Large random clusters never give mask 1 alone: five nodes, every one
    unschedulable, so a pod that does not tolerate it fails NodeUnschedulable on
    all of them and NodeAffinity is never asked."""
    nr, pr, ts, rq = cluster(5, 60, 6, 77)
    nr["unschedulable"] = 1
    return nr, pr, ts, rq, 77


def inloop_cluster():
    """Three nodes of raw score 30, 120, 250 (zones 1, 2, 3); node 0 carries the
    pod's name digit, so under weights (7, 1) it wins with 70 + its normalised
    score: 103 unfiltered ([33, 40, 100]), 110 when the requirement zone In [1, 3]
    drops node 1 ([40, 100])."""
    from minisched_amd import _lib

    full = (1 << 256) - 1
    nr = np.zeros(3, dtype=_lib.NODE_REC)
    nr["zone"], nr["name_digit"], nr["allowed_pods"] = [1, 2, 3], [3, 0xFF, 0xFF], 110
    pr = np.zeros(4, dtype=_lib.POD_REC)
    pr["ordinal"], pr["name_digit"], pr["pref_zone"] = np.arange(4), 3, 1
    ts = _lib.nam_term_sets_ext_array([[(30, 0b1110, full), (90, 0b1100, full), (100, 0b1000, full),
                                        (30, 0b1000, full)]])
    rq = _lib.nam_required_sets_array([[(0b1010, full)]])
    return nr, pr, ts, rq


def coverage(ref, unfiltered):
    """What the issue asks of the inputs, counted on a reference: pods per
    FitError mask, and SUCCESS pods whose winner differs from the unfiltered run's."""
    un = ref["code"] == 2
    moved = (ref["code"] == 0) & (unfiltered["code"] == 0) & (ref["node"] != unfiltered["node"])
    return {m: int((un & (ref["mask"] == m)).sum()) for m in (1, 8, 9)}, int(moved.sum())
