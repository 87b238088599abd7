"""Engine.explain_sharded (ms_explain_sharded / ms_explain_sharded_device) on
contexts joined to a communicator, against tests/_explain_ref.py over the WHOLE
cluster. Runs on the TEST-ONLY loopback library: G contexts on one GPU, one host
thread per rank, a bounded join (tests/test_gpu_loopback.py's run_ranks).

A case of tests/_explain_cases.py is cut into G contiguous shards at `cuts` (row
indices of the case): rank r owns rows [cut[r], cut[r + 1]) as the ordinals
node_base + row, upserts its part of the nodes, deletes its part of the dead
rows, joins, and calls explain_sharded over its whole range. Its rows must equal
the reference's columns [cut[r], cut[r + 1]) and every rank's summaries the
reference's whole-cluster summaries, element for element (integers: no
tolerance). The cuts lie where the shards' records meet: between the
TaintToleration census's first three / last entries, at the NodeAffinity anchor,
before the one rescaling node, inside a run of rescales, and around shards with
no present or no feasible row.
"""
import numpy as np
import pytest

import _explain_cases as cases
import _explain_ref as ref
from minisched_amd import _lib
from minisched_amd._lib import MODE_BATCHED, Engine
from test_gpu_loopback import lb, run_ranks  # noqa: F401  (lb: the loopback library fixture)

pytestmark = pytest.mark.gpu
T = cases.T
RANK_TIMEOUT = 150  # above the loopback rendezvous' own 120 s: a rank that never calls is reported by the library


def _engine(lib, c, lo, hi):
    """The context of rows [lo, hi) of the case (the dead rows upserted, then deleted), not joined."""
    ps, base = c["plugin_set"], c["node_base"]
    e = Engine(max_nodes=hi - lo, plugin_set=ps, node_base=base + lo, seed=c["seed"],
               score_weights=c["weights"] if ps in (2, 4) else (0, 0), lib=lib)
    up = min(hi, len(c["nodes"]))
    if up > lo:
        e.upsert(base + np.arange(lo, up), c["nodes"][lo:up])
    dead = c["dead"][(c["dead"] >= lo) & (c["dead"] < hi)]
    if len(dead):
        e.delete(base + dead)
    if ps == 4:
        e.nam_term_sets_ext(c["term_sets"])
        e.nam_required_sets(c["req_sets"])
    return e


def _edges(c, cuts):
    edges = [0] + list(cuts) + [c["max_nodes"]]
    assert all(a < b for a, b in zip(edges, edges[1:])), edges
    return edges


def run_sharded(lib, c, cuts, fn):
    """fn(engine, rank, lo, hi) on every rank's joined context; the per-rank results."""
    edges = _edges(c, cuts)
    G = len(edges) - 1
    cid = _lib.comm_id_create(lib)

    def rank_fn(r):
        lo, hi = edges[r], edges[r + 1]
        with _engine(lib, c, lo, hi) as e:
            e.comm_init(cid, r, G)
            return fn(e, r, lo, hi)

    return edges, run_ranks(G, rank_fn, timeout=RANK_TIMEOUT)


def check_whole(lib, c, cuts, pods=None, tag=None):
    """Every rank explains its whole range; rows and summaries against the reference."""
    want_rows, want_sums = cases.reference(c)
    p = c["pods"] if pods is None else pods
    edges, got = run_sharded(lib, c, cuts, lambda e, r, lo, hi: e.explain_sharded(p))
    for r, (rows, sums) in enumerate(got):
        lo, hi = edges[r], edges[r + 1]
        assert rows.shape == (len(p), hi - lo)
        ref.same(rows, sums, want_rows[:len(p), lo:hi], want_sums[:len(p)],
                 f"{tag or c['tag']} G={len(edges) - 1} rank {r} rows [{lo}, {hi})")


# tag -> {G: cuts}
DIRECTED = {
    # the feasible spots 5, T - 1, T, 2T + 3, 2T + 36 fall on three ranks: the first three and the last
    # entry and the rank parity all cross shards
    **{f"tt F={F}": {3: (T, 2 * T + 3), 2: (T,)} for F in range(6)},
    "tt [1, 0]": {2: (1,)},  # [100, 100]: the smallest shape at which a missing cross-shard census shows
    "tt counts 0..8": {3: (3, 64), 2: (3,)},  # a shard with fewer than four feasible rows
    "nam KAT filtered=False": {3: (1, 2), 2: (1,)},
    "nam KAT filtered=True": {3: (1, 2), 2: (1,)},
    # the raw 250 node is the first row of the last rank and rescales every row of the earlier ranks;
    # the raw 101 run [T + 10, T + 50) is split by a cut
    "nam late rescale": {3: (T + 30, 2 * T + 20), 2: (2 * T + 20,)},
    "nam x101": {2: (100,), 3: (100, 200)},
    # the anchor T + 7 is the first row of rank 1, rank 0 has none, rank 2 holds zone-3 rows that must not read 100
    "na anchor": {3: (T + 7, 2 * T + 2), 2: (T + 7,)},
    "la pairs": {2: (64,), 3: (64, 129)},
}


@pytest.mark.parametrize("tag,G", [(t, G) for t, by_g in DIRECTED.items() for G in sorted(by_g)])
def test_directed(lb, tag, G):
    c = cases.all_cases()[tag]
    if tag.startswith("nam KAT"):
        assert c["max_nodes"] == 3
    check_whole(lb, c, DIRECTED[tag][G])


# Cuts at T and 2T: under 90 % tombstones rank 1 holds no present row at all (an empty shard) and rank 2
# only unschedulable rows. The 65-row table has no such edges: a short first shard and a one-row last one.
FAMILY = [(f"n={2 * T + 37} dead=0% base=33333", (T, 2 * T)), (f"n={2 * T + 37} dead=90% base=0", (T, 2 * T)),
          ("n=65 dead=90% base=33333", (3, 64)), ("n=5 dead=0% base=0", (1, 2, 3, 4))]


@pytest.mark.parametrize("ps", range(5))
@pytest.mark.parametrize("tag,cuts", FAMILY)
def test_family(lb, ps, tag, cuts):
    check_whole(lb, cases.all_cases()[f"set{ps} {tag}"], cuts)


def test_windows_and_outputs_differ_per_rank(lb):
    # rank 0: rows only, ten rows straddling a tile edge; rank 1: summaries only; rank 2: both NULL. The
    # collectives of the call are those of a call where every rank asks for everything.
    c = cases.all_cases()["nam late rescale"]
    cuts = DIRECTED["nam late rescale"][3]
    want_rows, want_sums = cases.reference(c)
    base, a = c["node_base"], T - 5

    def mixed(e, r, lo, hi):
        if r == 0:
            return e.explain_sharded(c["pods"], first=base + a, n_nodes=10, summaries=False)
        if r == 1:
            return e.explain_sharded(c["pods"], rows=False)
        return e.explain_sharded(c["pods"], rows=False, summaries=False)

    n0 = lb.lb_collectives_issued()
    check_whole(lb, c, cuts)
    n1 = lb.lb_collectives_issued()
    edges, got = run_sharded(lb, c, cuts, mixed)
    n2 = lb.lb_collectives_issued()
    assert edges[1] > a + 10  # the window lies inside rank 0's range
    assert n1 - n0 == n2 - n1 == 2, (n0, n1, n2)
    assert got[0][1] is None and got[1][0] is None and got[2] == (None, None)
    ref.same(got[0][0], None, want_rows[:, a:a + 10], None, "rank 0: rows only")
    ref.same(want_rows, got[1][1], want_rows, want_sums, "rank 1: summaries only")


def test_host_array_chunks(lb):
    # ms_explain_sharded's row staging holds 64 MiB: 256 pods x 10,923 rows x 24 B is the least that
    # takes two chunks (255 pods + 1) on rank 0, while rank 1 (65 rows) takes one; the collectives are
    # the same two on both
    n0, n1 = 10_923, 65
    assert 256 * n0 * _lib.EXPLAIN_ROW.itemsize > 64 << 20 >= 256 * (n0 - 1) * _lib.EXPLAIN_ROW.itemsize
    pods = np.concatenate([cases.base_pods(0, 71)] * 7)[:256].copy()
    pods["ordinal"] = np.arange(256)
    c = cases.case(0, cases.base_nodes(0, n0 + n1, 71), pods, node_base=1000, seed=71, tag="chunks")
    before = lb.lb_collectives_issued()
    check_whole(lb, c, (n0,))
    assert lb.lb_collectives_issued() - before == 2


@pytest.mark.parametrize("ps", range(5))
def test_summary_decodes_to_the_scheduling_result(lb, ps):
    # best_key (the maximum over the shards) and the summed counts decode to what ms_schedule_batch
    # returns on the same joined contexts afterwards
    c = cases.all_cases()[f"set{ps} n={2 * T + 37} dead=0% base=33333"]
    pods = c["pods"]

    def fn(e, r, lo, hi):
        _, sums = e.explain_sharded(pods, rows=False)
        return sums, e.schedule(pods, MODE_BATCHED)

    _, got = run_sharded(lb, c, (T, 2 * T), fn)
    for r, (sums, res) in enumerate(got):
        for j in range(len(pods)):
            assert ref.decode(sums[j]) == (res["node"][j], res["score"][j], res["code"][j], res["plugin_mask"][j]), (r, j)


def test_argument_errors_issue_no_collective(lb):
    c = cases.all_cases()["set0 n=65 dead=0% base=33333"]
    many = np.concatenate([c["pods"]] * 7)[:257]
    before = lb.lb_collectives_issued()
    with _engine(lb, c, 0, 65) as e:  # not joined: refused as such, whatever else the call asks
        for kw in (dict(pods=c["pods"]), dict(pods=c["pods"][:3], first=c["node_base"] + 1, n_nodes=65), dict(pods=many)):
            with pytest.raises(_lib.MSError) as x:
                e.explain_sharded(**kw)
            assert x.value.code == _lib.MS_E_INVAL
            assert "single-shard" in str(x.value) and "ms_explain_device" in str(x.value)

    def fn(e, r, lo, hi):
        codes = []
        base = c["node_base"]
        for kw in (dict(pods=many), dict(pods=c["pods"][:3], first=base + lo + 1, n_nodes=hi - lo),
                   dict(pods=c["pods"][:3], first=base + lo - 1, n_nodes=2)):
            with pytest.raises(_lib.MSError) as x:
                e.explain_sharded(**kw)
            codes.append(x.value.code)
        rows, sums = e.explain_sharded(c["pods"][:0])  # no pods: MS_OK, no collective
        assert rows.shape == (0, hi - lo) and len(sums) == 0
        return codes

    _, got = run_sharded(lb, c, (30,), fn)
    assert got == [[_lib.MS_E_INVAL, _lib.MS_E_CAPACITY, _lib.MS_E_CAPACITY]] * 2
    assert lb.lb_collectives_issued() == before


@pytest.mark.parametrize("tag", ["tt F=5", "nam late rescale"])
def test_world_one_equals_the_single_context_call(lb, tag):
    c = cases.all_cases()[tag]
    with _engine(lb, c, 0, c["max_nodes"]) as e:
        rows0, sums0 = e.explain(c["pods"])
    with _engine(lb, c, 0, c["max_nodes"]) as e:
        e.comm_init(_lib.comm_id_create(lb), 0, 1)
        rows1, sums1 = e.explain_sharded(c["pods"])
    ref.same(rows1, sums1, rows0, sums0, f"{tag} world 1")


def test_repeat_call_grows_the_scratch(lb):
    # two calls on the same joined contexts, the second with more pods and a wider window: the scratch
    # with the gathered records grows in live contexts
    c = cases.all_cases()["nam late rescale"]
    want_rows, want_sums = cases.reference(c)

    def fn(e, r, lo, hi):
        first = e.explain_sharded(c["pods"][:5], n_nodes=1)
        return first, e.explain_sharded(c["pods"])

    edges, got = run_sharded(lb, c, DIRECTED["nam late rescale"][3], fn)
    for r, ((rows_a, sums_a), (rows_b, sums_b)) in enumerate(got):
        lo, hi = edges[r], edges[r + 1]
        ref.same(rows_a, sums_a, want_rows[:5, lo:lo + 1], want_sums[:5], f"rank {r}: 5 pods")
        ref.same(rows_b, sums_b, want_rows[:, lo:hi], want_sums, f"rank {r}: 40 pods")


def test_device_form_on_a_caller_stream(lb):
    # ms_explain_sharded_device on device-resident pods and a caller stream, nothing synchronised by the library
    import torch

    c = cases.all_cases()["na anchor"]
    want_rows, want_sums = cases.reference(c)
    pods = c["pods"]
    dev = torch.device("cuda:0")
    host_pods = pods.view(np.uint8).copy()

    def fn(e, r, lo, hi):
        n = hi - lo
        pods_d = torch.from_numpy(host_pods).to(dev)
        rows_d = torch.zeros(len(pods) * n * 24, dtype=torch.uint8, device=dev)
        sums_d = torch.zeros(len(pods) * 32, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()  # (the copies ran on torch's stream, not the caller stream below)
        s = torch.cuda.Stream(device=dev)
        e.explain_sharded_device(len(pods), pods_d.data_ptr(), c["node_base"] + lo, n, rows_d.data_ptr(),
                                 sums_d.data_ptr(), s.cuda_stream)
        s.synchronize()
        return (rows_d.cpu().numpy().view(_lib.EXPLAIN_ROW).reshape(len(pods), n),
                sums_d.cpu().numpy().view(_lib.EXPLAIN_SUMMARY))

    edges, got = run_sharded(lb, c, DIRECTED["na anchor"][3], fn)
    for r, (rows, sums) in enumerate(got):
        ref.same(rows, sums, want_rows[:, edges[r]:edges[r + 1]], want_sums, f"device form rank {r}")
