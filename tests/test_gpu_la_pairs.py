"""LeastAllocated and NodeResourcesFit of MS_PLUGINS_NU_NRF_NN_LA pair by pair
on the GPU, in every form the kernels evaluate them (ms_rows.h, ms_seq.hip).

The other GPU tests compare winners of whole queues; a score that is off by one
on a node that does not win, or only at capacities synth never draws, changes
nothing they see. Here every pod has exactly one feasible node (tests/_la_cases.py:
the Fit columns address it, the LeastAllocated columns carry the probed
(cap, nz, n)), so each result IS one pair's arithmetic, and every comparison is
exact equality with the Python-integer model (tests/test_la_cases.py proves that
model equal to the C oracle on the same tables, without a GPU). Every generated
pair is asserted, on both sides of every k * cap / 100 step.

Which form runs is not observable through the ABI (apart from seq_recomputes);
it follows from the selection code (sweep_rows_task, sweep_tp_task, rows_huge,
launch_sweep_full_tiles) and the table kinds of _la_cases:
  form 1  general, f32 estimate + one int64 compare: every batched test; the
          candidates and the sequential engine on the `general` and `slowpods`
          tables and with MINISCHED_SEQ_FAST=0
  form 2  the same compiled with the huge-row branch: the `huge` tables
  form 3  binary64, lane = row: the candidates on the `fast` tables (and the
          first batch of every sequential call)
  form 4  binary64, transposed, from derived rows: schedule(SEQUENTIAL) on the
          `fast` tables
  form 5  the validators' re-evaluation from a record plus the batch's binds:
          the walks (one node, every bind moves it to the next probe point)
Tested domain: capacities up to 2^56, NonZeroRequested >= 0, pod requests below
2^62 (beyond it the reference's own int64 arithmetic wraps; not pinned).
"""
import numpy as np
import pytest

import _la_cases as lc
from minisched_amd import _lib
from minisched_amd._lib import MODE_SEQUENTIAL, NODE_REC, PLUGINS_NU_NRF_NN_LA, POD_REC, RESULT, SEQ_CAND, SEQ_TOPK, Engine

pytestmark = pytest.mark.gpu

BIND_FIELDS = ("pod_count", "req_milli_cpu", "req_memory", "nonzero_milli_cpu", "nonzero_memory")
REC_FIELDS = ("alloc_milli_cpu", "alloc_memory", "req_milli_cpu", "req_memory", "nonzero_milli_cpu", "nonzero_memory",
              "allowed_pods", "pod_count")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    _lib.load()
    if _lib.device_count() == 0:
        pytest.fail("gpu test collected on a host without a visible device")


@pytest.fixture(scope="module")
def gpu():
    import torch

    class G:
        dev = torch.device("cuda:0")
        stream = torch.cuda.Stream(device=dev)
        sp = stream.cuda_stream

        @staticmethod
        def put(a):
            return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(G.dev)

        @staticmethod
        def buf(nbytes, fill=0xAB):
            return torch.full((nbytes,), fill, dtype=torch.uint8, device=G.dev)

        @staticmethod
        def get(t, dtype):
            G.stream.synchronize()
            return t.cpu().numpy().view(dtype)

    return G


def tables(kind):
    return lc.tables(kind, NODE_REC, POD_REC)[1]


def engine_for(tabs, max_batch=1 << 16):
    return Engine(max_nodes=tabs[0].M, plugin_set=PLUGINS_NU_NRF_NN_LA, seed=lc.SEED, max_batch=max_batch)


def load(e, t):
    """Replaces the whole table (and with it the binds of the previous one)."""
    e.upsert(np.arange(t.M), t.nodes)
    e.flush()


def same(what, got, want, t, where=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = np.nonzero(got != want)[0]
    if len(bad):
        p = int(bad[0])
        raise AssertionError(f"{what}: gpu {got[p]} model {want[p]} ({len(bad)} differ) "
                             f"{where(p) if where else lc.describe(t, p)}")


def same_results(res, t, what):
    for f, want in (("node", t.node), ("code", t.code), ("score", t.score), ("plugin_mask", t.mask)):
        same(f"{what} {f}", res[f], want, t)
    assert not res["_pad"].any()


# ---- forms 1 and 2: the batched sweep ---------------------------------------------
@pytest.mark.parametrize("kind", lc.KINDS)
def test_batched_pairs(gpu, kind):
    # k_sweep_full evaluates every wave with eval_full<false>, or eval_full<true> where
    # rows_huge ballots (the `huge` tables: a 2^53 decoy in every 16 rows, so in every
    # wave's 256): ms_select_batch_device for (node, code, score, mask), ms_sweep_device
    # for whole keys (1 = nothing feasible here but a node is listed) and the filter bytes
    tabs = tables(kind)
    with engine_for(tabs) as e:
        for t in tabs:
            load(e, t)
            n = len(t.pods)
            pods, res, keys, flags = gpu.put(t.pods), gpu.buf(24 * n), gpu.buf(8 * n), gpu.buf(4 * n)
            e.select_batch_device(n, pods.data_ptr(), res.data_ptr(), gpu.sp)
            e.sweep_device(n, pods.data_ptr(), keys.data_ptr(), flags.data_ptr(), gpu.sp)
            same_results(gpu.get(res, RESULT), t, "select_batch")
            same("sweep key", gpu.get(keys, np.uint64), np.where(t.key == 0, 1, t.key), t)
            same("sweep flags", gpu.get(flags, np.uint32), t.flags, t)


@pytest.mark.parametrize("name", sorted(lc.REGRESSIONS))
def test_regression_triples(gpu, name):
    # triples a form once got wrong (tests/_la_cases.py names the cause), mirrored, in a `general`
    # and a `huge` table: batched (forms 1, 2), candidates and schedule(SEQUENTIAL)
    chunk = [(t, t) for t in lc.REGRESSIONS[name]]
    for kind in ("general", "huge"):
        t = lc.build_table(kind, chunk, NODE_REC, POD_REC)
        with Engine(max_nodes=t.M, plugin_set=PLUGINS_NU_NRF_NN_LA, seed=lc.SEED) as e:
            load(e, t)
            n = len(t.pods)
            pods, res = gpu.put(t.pods), gpu.buf(24 * n)
            e.select_batch_device(n, pods.data_ptr(), res.data_ptr(), gpu.sp)
            same_results(gpu.get(res, RESULT), t, f"{name} select_batch[{kind}]")
            c, f = _candidates(gpu, e, t)
            _check_candidates(c, f, t, f"{name} candidates[{kind}]")
            same_results(e.schedule(t.pods, MODE_SEQUENTIAL), t, f"{name} sequential[{kind}]")


# ---- form 3 and its fallbacks: the candidates --------------------------------------
def _candidates(gpu, e, t):
    n = len(t.pods)
    cb = SEQ_CAND.itemsize * SEQ_TOPK
    pods, cands, flags = gpu.put(t.pods), gpu.buf(cb * n), gpu.buf(4 * n)
    for a in range(0, n, _lib.SEQ_SHARD_BATCH_MAX):
        nb = min(_lib.SEQ_SHARD_BATCH_MAX, n - a)
        e.seq_candidates_device(nb, pods.data_ptr() + 40 * a, cands.data_ptr() + cb * a, flags.data_ptr() + 4 * a,
                                gpu.sp)
    return gpu.get(cands, SEQ_CAND).reshape(n, SEQ_TOPK), gpu.get(flags, np.uint32)


def _check_candidates(c, f, t, what):
    same(f"{what} cands[0].key", c["key"][:, 0], t.key, t)
    for r in range(1, SEQ_TOPK):
        same(f"{what} cands[{r}].key", c["key"][:, r], np.zeros(len(t.pods), np.uint64), t)
    same(f"{what} flags", f, t.flags, t)
    # the candidate's record is the node's (all zero where there is no candidate)
    won = t.code == lc.CODE_SUCCESS
    rows = np.where(won, t.node, 0)
    for fld in REC_FIELDS:
        same(f"{what} cands[0].{fld}", c[fld][:, 0], np.where(won, t.nodes[fld][rows], 0), t)
    fd = t.nodes["unschedulable"].astype(np.uint32) | (t.nodes["name_digit"].astype(np.uint32) << 8)
    same(f"{what} cands[0].flags_digit", c["flags_digit"][:, 0], np.where(won, fd[rows], 0), t)
    assert not c["_pad"].any()
    for fld in REC_FIELDS + ("flags_digit",):
        assert not c[fld][:, 1:].any(), fld


@pytest.mark.parametrize("kind,fast", [("fast", None), ("general", None), ("huge", None), ("slowpods", None),
                                       ("fast", "0")])
def test_candidates_pairs(gpu, monkeypatch, kind, fast):
    # ms_seq_candidates_device sweeps lane = row (k_sweep_full_topk, no derived rows):
    # eval_fast on the `fast` tables; eval_full<false> where a row (`general`) or a pod
    # (`slowpods`) of the wave's task is outside the binary64 range or MINISCHED_SEQ_FAST=0
    # turns the fast form off; eval_full<true> on the `huge` tables
    if fast is not None:
        monkeypatch.setenv("MINISCHED_SEQ_FAST", fast)
    tabs = tables(kind)
    with engine_for(tabs) as e:
        for t in tabs:
            load(e, t)
            c, f = _candidates(gpu, e, t)
            _check_candidates(c, f, t, f"candidates[{kind}]")


# ---- form 4: the sequential engine's transposed sweep ----------------------------------
@pytest.mark.parametrize("kind,batch", [("fast", None), ("fast", "1"), ("fast", "7"), ("general", None),
                                        ("huge", None), ("slowpods", None)])
def test_sequential_pairs(kind, batch, monkeypatch):
    # schedule(SEQUENTIAL): the first batch of a call is swept lane = row, every later one
    # by sweep_tp_task inside the step (eval_tp64 on the derived rows k_build_drows made);
    # `general` / `huge` tiles and `slowpods` groups fall back to sweep_rows_task_lean.
    # Each node is addressed by one pod of the call, so no winner is stale: every score
    # comes from a sweep, none from the validator (seq_recomputes stays 0). 1000 probe rows
    # are several tiles with a short last one on any part (tiles: 64..256 rows).
    if batch is not None:
        monkeypatch.setenv("MINISCHED_SEQ_BATCH", batch)
    tabs = tables(kind)
    with engine_for(tabs) as e:
        for t in tabs:
            load(e, t)
            same_results(e.schedule(t.pods, MODE_SEQUENTIAL), t, f"sequential[{kind}]")
            back, want = e.read(0, t.M), lc.after_binds(t)
            for fld in BIND_FIELDS:
                same(f"table {fld}", back[fld], want[fld], t, where=lambda r: f"row {r}")
        info = e.info()
        assert info.seq_pods > 0
        assert info.seq_recomputes == 0 and info._pad == 0


# ---- form 5: the validators' re-evaluation ------------------------------------------------
def _walk_node(cap, digit, n_pods):
    nr = np.zeros(1, dtype=NODE_REC)
    nr["alloc_milli_cpu"] = nr["alloc_memory"] = cap
    nr["allowed_pods"] = n_pods + 5
    nr["name_digit"] = digit
    return nr


def _walk_where(cap, pods):
    return lambda p: f"cap {cap} pod {p}: n = {int(pods['nonzero_milli_cpu'][p])}, nz before = " \
                     f"{int(pods['nonzero_milli_cpu'][:p].astype(object).sum())}"


@pytest.mark.parametrize("digit", [3, 0xFF])
def test_validator_walk(digit):
    # one node, pods with zero Fit requests whose non-zero requests walk NonZeroRequested
    # down the step points: the only candidate of every pod after the first of a batch was
    # bound earlier in it (or in the batch before), so its score is the validator's eval_full
    # on the record plus those binds (slot_row)
    with Engine(max_nodes=1, plugin_set=PLUGINS_NU_NRF_NN_LA, seed=lc.SEED) as e:
        for cap in lc.WALK_CAPS:
            pods, scores, nz = lc.walk(cap, POD_REC, digit, ordinal0=cap % 1000)
            before = e.info().seq_recomputes
            e.upsert(np.zeros(1, np.uint32), _walk_node(cap, digit, len(pods)))
            res = e.schedule(pods, MODE_SEQUENTIAL)
            same("walk code", res["code"], np.zeros(len(pods), np.int32), None, _walk_where(cap, pods))
            same("walk node", res["node"], np.zeros(len(pods), np.int32), None, _walk_where(cap, pods))
            same("walk score", res["score"], scores, None, _walk_where(cap, pods))
            back = e.read(0, 1)
            assert (back["nonzero_milli_cpu"][0], back["nonzero_memory"][0], back["pod_count"][0]) == (nz, nz, len(pods))
            assert (back["req_milli_cpu"][0], back["req_memory"][0]) == (0, 0)
            # every pod but the first of each batch (<= 128 pods) was re-evaluated
            assert e.info().seq_recomputes - before >= len(pods) - (len(pods) + 63) // 64
        assert e.info()._pad == 0


def test_validator_walk_replicated(gpu):
    # the same walk through ms_seq_candidates_device + ms_seq_validate_device (one shard):
    # k_seq_validate_rep re-evaluates a bound candidate from its live record (cand_row)
    import torch

    digit, batch = 7, 64
    cb = SEQ_CAND.itemsize * SEQ_TOPK
    with Engine(max_nodes=1, plugin_set=PLUGINS_NU_NRF_NN_LA, seed=lc.SEED) as e:
        for cap in lc.WALK_CAPS:
            pr, scores, nz = lc.walk(cap, POD_REC, digit, ordinal0=cap % 1000)
            n = len(pr)
            e.upsert(np.zeros(1, np.uint32), _walk_node(cap, digit, n))
            pods, cands, flags = gpu.put(pr), gpu.buf(cb * batch), gpu.buf(4 * batch)
            res, done = gpu.buf(24 * n), torch.zeros(1, dtype=torch.int32, device=gpu.dev)
            a = 0
            while a < n:
                nb = min(batch, n - a)
                e.seq_candidates_device(nb, pods.data_ptr() + 40 * a, cands.data_ptr(), flags.data_ptr(), gpu.sp)
                e.seq_validate_device(nb, pods.data_ptr() + 40 * a, 1, cands.data_ptr(), flags.data_ptr(),
                                      res.data_ptr() + 24 * a, done.data_ptr(), gpu.sp)
                gpu.stream.synchronize()
                assert int(done.item()) == nb  # one node, one listed candidate: every pod is decidable
                a += nb
            r = gpu.get(res, RESULT)
            same("walk code", r["code"], np.zeros(n, np.int32), None, _walk_where(cap, pr))
            same("walk score", r["score"], scores, None, _walk_where(cap, pr))
            back = e.read(0, 1)
            assert (back["nonzero_milli_cpu"][0], back["nonzero_memory"][0], back["pod_count"][0]) == (nz, nz, n)


# ---- NodeUnschedulable / NodeResourcesFit truth table ---------------------------------------
GIB = 1 << 30
# node: Allocatable 4000 m / 8 GiB, 110 pods; the case gives Requested, len(Pods), Unschedulable
# pod: (req cpu, req mem, tolerates); expected (feasible, mask of the pair's first failing plugin)
TRUTH = [
    # request equal to free and one above it, CPU alone and memory alone
    ("cpu == free", dict(req=(1500, 3 * GIB)), (2500, 0, 0), (True, 0)),
    ("cpu == free + 1", dict(req=(1500, 3 * GIB)), (2501, 0, 0), (False, 2)),
    ("mem == free", dict(req=(1500, 3 * GIB)), (0, 5 * GIB, 0), (True, 0)),
    ("mem == free + 1", dict(req=(1500, 3 * GIB)), (0, 5 * GIB + 1, 0), (False, 2)),
    ("both == free", dict(req=(1500, 3 * GIB)), (2500, 5 * GIB, 0), (True, 0)),
    ("cpu fits, mem one above", dict(req=(1500, 3 * GIB)), (1, 5 * GIB + 1, 0), (False, 2)),
    # over-committed node (negative free): a zero-request pod passes, a 1-unit pod fails
    ("negative free, zero request", dict(req=(5000, 9 * GIB)), (0, 0, 0), (True, 0)),
    ("negative free, 1 m cpu", dict(req=(5000, 3 * GIB)), (1, 0, 0), (False, 2)),
    ("negative free, 1 B mem", dict(req=(1500, 9 * GIB)), (0, 1, 0), (False, 2)),
    # AllowedPodNumber - len(Pods) of 1 and 0, zero and non-zero requests
    ("room 1, zero request", dict(req=(1500, 3 * GIB), count=109), (0, 0, 0), (True, 0)),
    ("room 1, request", dict(req=(1500, 3 * GIB), count=109), (100, GIB, 0), (True, 0)),
    ("room 0, zero request", dict(req=(1500, 3 * GIB), count=110), (0, 0, 0), (False, 2)),
    ("room 0, request", dict(req=(1500, 3 * GIB), count=110), (100, GIB, 0), (False, 2)),
    ("room -1, zero request", dict(req=(1500, 3 * GIB), count=111), (0, 0, 0), (False, 2)),
    # first-failure attribution: an unschedulable node that also does not fit
    ("unschedulable + no fit, intolerant", dict(req=(1500, 3 * GIB), unsched=1), (2501, 0, 0), (False, 1)),
    ("unschedulable + no fit, tolerant", dict(req=(1500, 3 * GIB), unsched=1), (2501, 0, 1), (False, 2)),
    ("unschedulable + full, intolerant", dict(req=(1500, 3 * GIB), unsched=1, count=110), (0, 0, 0), (False, 1)),
    ("unschedulable + fits, intolerant", dict(req=(1500, 3 * GIB), unsched=1), (2500, 0, 0), (False, 1)),
    ("unschedulable + fits, tolerant", dict(req=(1500, 3 * GIB), unsched=1), (2500, 5 * GIB, 1), (True, 0)),
]


def test_filter_truth_table(gpu):
    # a single present node (ordinal 37 of 64, the rest tombstoned): the pod's code and
    # plugin_mask, and the sweeps' filter bytes, are that pair's; batched, candidates, sequential
    ROW, N = 37, 64
    cb = SEQ_CAND.itemsize * SEQ_TOPK
    with Engine(max_nodes=N, plugin_set=PLUGINS_NU_NRF_NN_LA, seed=lc.SEED) as e:
        e.upsert(np.arange(N), np.zeros(N, dtype=NODE_REC))
        e.delete(np.delete(np.arange(N), ROW))
        for j, (name, nd, (rc, rm, tol), (feasible, mask)) in enumerate(TRUTH):
            nr = np.zeros(1, dtype=NODE_REC)
            nr["alloc_milli_cpu"], nr["alloc_memory"], nr["allowed_pods"] = 4000, 8 * GIB, 110
            nr["req_milli_cpu"], nr["req_memory"] = nd["req"]
            nr["nonzero_milli_cpu"], nr["nonzero_memory"] = 1700, 3 * GIB + 12345
            nr["pod_count"], nr["unschedulable"], nr["name_digit"] = nd.get("count", 10), nd.get("unsched", 0), 4
            pr = np.zeros(1, dtype=POD_REC)
            pr["ordinal"], pr["name_digit"], pr["tolerates_unschedulable"] = 900 + j, 4 if j % 2 else 5, tol
            pr["req_milli_cpu"], pr["req_memory"] = rc, rm
            pr["nonzero_milli_cpu"], pr["nonzero_memory"] = max(rc, 100), max(rm, 200 << 20)
            assert lc.filter_pair(nr[0], pr[0]) == (feasible, mask), name  # the model agrees with the table
            score = lc.pair_score((4000, 1700, int(pr["nonzero_milli_cpu"][0])),
                                  (8 * GIB, 3 * GIB + 12345, int(pr["nonzero_memory"][0])), 10 if j % 2 else 0)
            want = (ROW, 0, score, 0) if feasible else (-1, 2, 0, mask)
            key = lc.key_of(score, lc.SEED, 900 + j, ROW) if feasible else 0
            wflags = {0: 0, 1: 0x001, 2: 0x100}[mask]
            e.upsert(np.array([ROW]), nr)
            e.flush()
            pods, res, keys, flags = gpu.put(pr), gpu.buf(24), gpu.buf(8), gpu.buf(4)
            cands, cflags = gpu.buf(cb), gpu.buf(4)
            e.select_batch_device(1, pods.data_ptr(), res.data_ptr(), gpu.sp)
            e.sweep_device(1, pods.data_ptr(), keys.data_ptr(), flags.data_ptr(), gpu.sp)
            e.seq_candidates_device(1, pods.data_ptr(), cands.data_ptr(), cflags.data_ptr(), gpu.sp)
            r = gpu.get(res, RESULT)[0]
            assert (r["node"], r["code"], r["score"], r["plugin_mask"], r["_pad"]) == want + (0,), f"batched: {name}"
            assert gpu.get(keys, np.uint64)[0] == (key or 1), f"sweep key: {name}"
            assert gpu.get(flags, np.uint32)[0] == wflags, f"sweep flags: {name}"
            c = gpu.get(cands, SEQ_CAND)
            assert c["key"].tolist() == [key, 0, 0, 0], f"candidates: {name}"
            assert gpu.get(cflags, np.uint32)[0] == wflags, f"candidates flags: {name}"
            r = e.schedule(pr, MODE_SEQUENTIAL)[0]
            assert (r["node"], r["code"], r["score"], r["plugin_mask"], r["_pad"]) == want + (0,), f"sequential: {name}"
            back = e.read(ROW, 1)[0]
            assert back["pod_count"] == nr["pod_count"][0] + (1 if feasible else 0), name
            assert back["req_milli_cpu"] == nr["req_milli_cpu"][0] + (rc if feasible else 0), name
            assert back["req_memory"] == nr["req_memory"][0] + (rm if feasible else 0), name
