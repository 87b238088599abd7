"""ms_explain on a context joined to a communicator is refused (MS_E_INVAL with
a message), as ms_select_batch_device is: a row's final scores would need the
other shards' LIST context. Runs on the TEST-ONLY loopback library (two
contexts on one GPU, one host thread each)."""
import os
import threading

import numpy as np
import pytest

from minisched_amd import _lib, synth

pytestmark = pytest.mark.gpu


def test_explain_is_refused_on_a_joined_context():
    if not os.path.exists(_lib.LOOPBACK_LIB_PATH):
        pytest.fail("libminisched_gpu_loopback.so is missing: `make -C mini-kube-scheduler_amd comm-loopback`")
    lib = _lib.load(_lib.LOOPBACK_LIB_PATH)
    G, n = 2, 64
    nr, pr = synth.nodes(n, seed=3), synth.pods(8, seed=3)
    cid = _lib.comm_id_create(lib)
    out, errs = [None] * G, [None] * G

    def rank(r):
        try:
            lo, hi = r * n // G, (r + 1) * n // G
            with _lib.Engine(max_nodes=hi - lo, node_base=lo, seed=3, lib=lib) as e:
                e.upsert(np.arange(lo, hi), nr[lo:hi])
                e.comm_init(cid, r, G)
                try:
                    e.explain(pr)
                except _lib.MSError as x:
                    out[r] = (x.code, str(x))
                try:
                    e.explain(pr, rows=False)
                except _lib.MSError as x:
                    out[r] += (x.code,)
        except BaseException as x:  # reported below
            errs[r] = repr(x)

    ts = [threading.Thread(target=rank, args=(r,), daemon=True) for r in range(G)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not any(t.is_alive() for t in ts) and not any(errs), errs
    for r in range(G):
        assert out[r] is not None and out[r][0] == _lib.MS_E_INVAL and out[r][2] == _lib.MS_E_INVAL, out[r]
        assert "sharded context" in out[r][1]
