"""ms_comm_plugin_set_supported: which plugin sets the collective calls of a
joined context serve. Exported by the product library and by the loopback
build; needs no context and no device (CPU-only)."""
import os

import pytest

from minisched_amd import _lib


@pytest.mark.parametrize("path", [_lib.LIB_PATH, _lib.LOOPBACK_LIB_PATH], ids=["product", "loopback"])
def test_comm_plugin_set_supported(path):
    assert os.path.exists(path), "make -C mini-kube-scheduler_amd"
    lib = _lib.load(path)
    assert hasattr(lib, "ms_comm_plugin_set_supported")
    for ps in range(5):  # NU+NN, resource-aware, NodeAffinity, TaintToleration, multi-term NodeAffinity
        assert lib.ms_comm_plugin_set_supported(ps) == 1, ps
        assert _lib.comm_plugin_set_supported(ps, lib) is True
    for ps in (-1, 5):
        assert lib.ms_comm_plugin_set_supported(ps) == 0, ps
        assert _lib.comm_plugin_set_supported(ps, lib) is False
