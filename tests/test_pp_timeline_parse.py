"""tools/pp_wg_timeline.py's parser and phase figures on a small synthetic buffer (CPU only):
two records of 3 workgroups x 4 waves in 16 wave slots, stamps laid out by hand."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import pp_wg_timeline as tl  # noqa: E402

STAMPS, SLOTS, WAVES, WGS = 48, 16, 4, 3
TICKS_PER_US = 100  # s_memtime at 100 MHz here, as s_memrealtime


def _wave(base, wv, empty=False):
    # one wave's stamps, in ticks: entry at base, barriers 1-4 after 1, 2, 3 and 5 us, a sweep of
    # two digits (slots 0 and 3) with switch waits of 0.5 and 0.25 us, the sweep's end after
    # 5 + 20 + wv us, its barrier at 30 us, the final pass at 31, the end at 32
    s = np.zeros(STAMPS, dtype=np.uint64)
    if empty:
        return s
    us = lambda x: np.uint64(base + int(x * TICKS_PER_US))  # noqa: E731
    s[tl.ENTRY], s[tl.BAR1], s[tl.BAR2], s[tl.BAR3], s[tl.BAR4] = us(0), us(1), us(2), us(3), us(5)
    s[tl.DIGIT0 + 0], s[tl.DIGIT0 + 1], s[tl.DIGIT0 + 2] = us(5), us(5.5), us(15)
    s[tl.DIGIT0 + 9], s[tl.DIGIT0 + 10], s[tl.DIGIT0 + 11] = us(15), us(15.25), us(25 + wv)
    s[tl.DIGIT0 + 14] = us(25 + wv)  # a digit without tiles in this wave: done only
    s[tl.SWEEP_END], s[tl.SWEEP_BAR], s[tl.FINAL], s[tl.END] = us(25 + wv), us(30), us(31), us(32)
    s[tl.REAL0], s[tl.REAL1] = np.uint64(7_000 + base), np.uint64(7_000 + base + 32 * 100)
    s[tl.HASHES] = 1000 * (wv + 1)
    return s


def _record(base, empty_wg=None):
    t = np.zeros((WGS, SLOTS, STAMPS), dtype=np.uint64)
    for g in range(WGS):
        for w in range(WAVES):
            t[g, w] = _wave(base + 10 * g, w, empty=g == empty_wg)
    hdr = struct.pack("<8I", tl.MAGIC, 1, WGS, WAVES, STAMPS, 104, 300, SLOTS)
    return hdr + t.tobytes()


def test_parse_records():
    recs = tl.parse(_record(1_000) + _record(9_000, empty_wg=2))
    assert len(recs) == 2
    r = recs[0]
    assert (r["workgroups"], r["waves"], r["stamps"], r["chunk"], r["pods"]) == (WGS, WAVES, STAMPS, 104, 300)
    assert r["t"].shape == (WGS, WAVES, STAMPS)
    assert r["t"][1, 2, tl.ENTRY] == 1_010 and r["t"][1, 2, tl.HASHES] == 3000
    assert not recs[1]["t"][2].any()


@pytest.mark.parametrize("cut", [10, 32 + 8, 32 + WGS * SLOTS * STAMPS * 8 + 5])
def test_parse_rejects_truncated(cut):
    with pytest.raises(ValueError):
        tl.parse((_record(1_000) + _record(2_000))[:cut])


def test_parse_rejects_bad_magic():
    with pytest.raises(ValueError):
        tl.parse(b"\0" * 4 + _record(1_000)[4:])


def test_phases():
    for rec in tl.parse(_record(1_000) + _record(9_000, empty_wg=2)):
        p = tl.phases(rec, ghz=2.0)
        assert p["memtime_mhz"] == pytest.approx(100.0)
        assert p["prologue_us"] == pytest.approx(5.0)
        assert p["barrier3_to_4_us"] == pytest.approx(2.0)
        assert p["planes_landed_after_barrier3_us"] is None  # never stamped
        assert p["switch_wait_sum_us"] == pytest.approx(0.75)
        # waves 0..3 hash for 20 .. 23 us less the 0.75 of waiting; the barrier waits mirror it
        assert p["hashing_us"] == pytest.approx(20.75)
        assert p["sweep_barrier_wait_us"] == pytest.approx(3.5)
        assert p["sweep_barrier_wait_by_simd_us"] == pytest.approx([5.0, 4.0, 3.0, 2.0])
        assert p["final_and_epilogue_us"] == pytest.approx(2.0)
        assert p["kernel_wave_us"] == pytest.approx(32.0)
        # one wave per SIMD: 1000 (wv + 1) hashes x 5.5 VALU x 4 cycles over (19.25 + wv) us at 2 GHz
        want = [1000 * (w + 1) * 5.5 * 4 / ((19.25 + w) * 2000) for w in range(4)]
        assert p["hash_issue_efficiency_by_simd"] == pytest.approx(want)
    assert tl.parse(_record(9_000, empty_wg=2))[0]["t"].shape[0] == WGS
    assert tl.phases(tl.parse(_record(9_000, empty_wg=2))[0], 2.0)["waves_recorded"] == (WGS - 1) * WAVES


def test_summarise_medians():
    recs = tl.parse(_record(1_000) + _record(5_000) + _record(9_000, empty_wg=0))
    s = tl.summarise(recs, ghz=2.0)
    assert s["records"] == 3 and s["prologue_us"] == pytest.approx(5.0)
    assert len(s["hash_issue_efficiency_by_simd"]) == 4
