"""MS_PLUGINS_NU_NN_NAM on the GPU, one row's normalised NodeAffinity score at
a time. Under score weights (11, 1) the one feasible row carrying a pod's name
digit wins outright, so the cycle returns F[class][row] itself: node = the row,
score = 110 + F. tests/_nam_probe_cases.py builds the tables, moves up to ten
such probes per state over them and holds the model of what must come back;
tests/test_nam_probe_cases.py proves that model against the C oracle's literal
loop and counts what the probes cover. Here every probe pod of every state is
compared exactly (node, code, score, plugin_mask) on one context (640 rows in
10 row segments, every row probed; 8,704 rows in 8 segments of two LDS tiles),
over node shards, through the chunked host call, with required sets, and under
weights (23, 2).
"""
import numpy as np
import pytest

import _nam_probe_cases as pc
import _nam_required_ref as ref
from minisched_amd import _lib

pytestmark = pytest.mark.gpu

NAM = _lib.PLUGINS_NU_NN_NAM


def _engine(t, weights=pc.W_PROBE, lo=0, hi=None, max_batch=1 << 16):
    hi = len(t.nodes) if hi is None else hi
    e = _lib.Engine(max_nodes=max(1, hi - lo), plugin_set=NAM, node_base=lo, seed=pc.SEED, score_weights=weights,
                    max_batch=max_batch)
    e.nam_term_sets_ext(t.ts)
    if t.rq is not None:
        e.nam_required_sets(t.rq)
    e.upsert(np.arange(lo, hi), t.nodes[lo:hi])
    gone = np.asarray([d for d in t.dead if lo <= d < hi], dtype=np.uint32)
    if len(gone):
        e.delete(gone)
    e.flush()
    return e


def _move_probes(e, t, old, new, lo=0, hi=None):
    """The probes from the rows `old` to the rows `new`: an upsert of the changed
    rows of this context; the table, the term sets and the engine stay."""
    hi = len(t.nodes) if hi is None else hi
    nr = t.with_digits(new)
    rows = np.asarray(sorted(r for r in set(old) | set(new) if lo <= r < hi and r not in t.dead), dtype=np.int64)
    if len(rows):
        e.upsert(rows, nr[rows])
        e.flush()
    return nr


def _device_cycle(e, pr):
    import torch

    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    pods = torch.from_numpy(pr.view(np.uint8).copy()).to(dev)
    out = torch.full((len(pr) * 24,), 0xCD, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # (the fill ran on torch's stream, not s)
    e.select_batch_device(len(pr), pods.data_ptr(), out.data_ptr(), s.cuda_stream)
    s.synchronize()
    return out.cpu().numpy().view(_lib.RESULT)


def _check(res, want, name, targets, pr, tag, weights=pc.W_PROBE, only=None):
    idx = np.arange(len(pr)) if only is None else np.nonzero(only)[0]
    for k_res, k in (("node", "node"), ("code", "code"), ("score", "score"), ("plugin_mask", "mask")):
        got, exp = np.asarray(res[k_res]).astype(np.int64)[idx], np.asarray(want[k]).astype(np.int64)[idx]
        if not np.array_equal(got, exp):
            bad = idx[np.nonzero(got != exp)[0][:6]]
            what = [dict(pc.describe(name, targets, pr, int(j), res["score"][j], weights), pod=int(j),
                         got=int(res[k_res][j]), want=int(want[k][j])) for j in bad]
            raise AssertionError(f"{tag}: {k} differs for {int((got != exp).sum())} pods, first {what}")


def _against_oracle(oracle, res, t, nr, pr, miss, weights, tag):
    """The pods whose target is infeasible for their class: the full reference
    result, tie-break included (the oracle's literal loop; with required sets the
    tombstone reference)."""
    j = np.nonzero(miss)[0]
    if len(j) == 0:
        return
    nr = nr.copy()
    nr["allowed_pods"][np.asarray(t.dead, dtype=np.int64)] = -1
    if t.rq is not None:
        o = ref.schedule_tombstone(oracle, nr, pr[j], t.ts, t.rq, weights=weights, seed=pc.SEED, literal=True)
    else:
        o = oracle.schedule_nam_ext(nr, pr[j], t.ts, weights=weights, literal=True, seed=pc.SEED)
    ref.same(res[j], o, tag + " (infeasible targets, oracle)")


@pytest.mark.parametrize("name,weights", [("all_rows", pc.W_PROBE), ("required", pc.W_PROBE), ("w23_2", (23, 2))])
def test_probes_on_one_context(oracle, name, weights):
    base = pc.base_table(name)
    t = pc.table(base)
    pr = t.pods()
    old = []
    with _engine(t, weights) as e:
        for s, targets in enumerate(pc.states(name)):
            nr = _move_probes(e, t, old, targets)
            old = targets
            want = pc.expect(base, targets, pr, weights=weights)
            res = _device_cycle(e, pr)
            _check(res, want, base, targets, pr, f"{name} state {s}", weights)
            _against_oracle(oracle, res, t, nr, pr, ~want["hit"], weights, f"{name} state {s}")


@pytest.mark.parametrize("part", [0, 1, 2])
def test_probes_on_two_tile_segments(part):
    # 8,704 rows, 1,202 classes: 8 row segments of 1,088 rows, each two LDS tiles (1,024 + 64)
    # in k_nam_seg's forward and k_nam_fscore's reverse tile loop; 4 of the 12 states per case
    t = pc.table("multi_tile")
    pr = t.pods()
    old = []
    with _engine(t) as e:
        for s, targets in list(enumerate(pc.states("multi_tile")))[part::3]:
            _move_probes(e, t, old, targets)
            old = targets
            want = pc.expect("multi_tile", targets, pr)
            _check(_device_cycle(e, pr), want, "multi_tile", targets, pr, f"multi_tile state {s}", only=want["hit"])


def test_probes_through_the_chunked_host_call(oracle):
    # ms_schedule_batch in chunks of 700 pods: the 1,320 pods straddle two chunks, classes too
    t = pc.table("all_rows")
    pr = t.pods()
    old = []
    with _engine(t, max_batch=700) as e:
        for s, targets in enumerate(pc.states("host_chunks")):
            nr = _move_probes(e, t, old, targets)
            old = targets
            want = pc.expect("all_rows", targets, pr)
            res = e.schedule(pr, _lib.MODE_BATCHED)
            _check(res, want, "all_rows", targets, pr, f"host chunks state {s}")
            _against_oracle(oracle, res, t, nr, pr, ~want["hit"], pc.W_PROBE, f"host chunks state {s}")


def _shard_cycle(engines, pr):
    import torch

    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    pods = torch.from_numpy(pr.view(np.uint8).copy()).to(dev)
    G, P, SB = len(engines), len(pr), _lib.NAM_SEG_BYTES
    segs = torch.zeros(G * P * SB, dtype=torch.uint8, device=dev)
    keys = torch.zeros((G, P), dtype=torch.int64, device=dev)
    out = torch.zeros(P * 24, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # (the fills ran on torch's stream, not s)
    for g, e in enumerate(engines):
        e.nam_segment_device(P, pods.data_ptr(), segs.data_ptr() + g * P * SB, s.cuda_stream)
    for g, e in enumerate(engines):
        e.nam_keys_device(P, pods.data_ptr(), G, g, segs.data_ptr(), keys[g].data_ptr(), s.cuda_stream)
    s.synchronize()
    best = keys.max(dim=0).values.contiguous()  # keys < 2^63: the signed max is the unsigned one
    present = sum(int(e.info().present_nodes) for e in engines)
    torch.cuda.synchronize()
    engines[0].decode_device(P, pods.data_ptr(), best.data_ptr(), 0, present, out.data_ptr(), s.cuda_stream)
    s.synchronize()
    return out.cpu().numpy().view(_lib.RESULT)


@pytest.mark.parametrize("name", ["shards", "multi_tile"])
def test_probes_over_node_shards(oracle, name):
    # nam_segment_device -> nam_keys_device (the later shards' table `after`, the earlier
    # shards' non-zero node `m_in`) -> max -> decode_device. shards: a one-row shard whose
    # row is deleted, cuts inside a row segment; multi_tile: two shards cut off the 64-row grid
    t = pc.table(name)
    pr = t.pods()
    cuts = pc.SHARD_CUTS if name == "shards" else (0, pc.MULTI_TILE_CUT, len(t.nodes))
    st = pc.states("shards") if name == "shards" else pc.multi_tile_shard_states()
    engines = [_engine(t, lo=lo, hi=hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    try:
        old = []
        for s, targets in enumerate(st):
            for e, lo, hi in zip(engines, cuts[:-1], cuts[1:]):
                nr = _move_probes(e, t, old, targets, lo, hi)
            old = targets
            want = pc.expect(name, targets, pr)
            res = _shard_cycle(engines, pr)
            if name == "shards":
                _check(res, want, name, targets, pr, f"shards state {s}")
                _against_oracle(oracle, res, t, nr, pr, ~want["hit"], pc.W_PROBE, f"shards state {s}")
            else:
                _check(res, want, name, targets, pr, f"multi_tile shards state {s}", only=want["hit"])
    finally:
        for e in engines:
            e.close()
