"""Host side of the batched simulators (no GPU): the workgroup table of k_bloch_batch / k_abr_batch, the bindings, and the
argument errors that mbfir.bloch_batch / abr_batch / sim_rf_scale_batch raise before any device work."""
import os
import re

import numpy as np
import pytest

import mbfir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mbfir.h")).read()
    for sym, nargs in (("mbfir_bloch_batch", 27), ("mbfir_abr_batch", 16), ("mbfir_test_sim_blocks", 5)):
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert len(mbfir.SYMBOLS[sym][1]) == nargs, sym
    for name in ("bloch_batch", "abr_batch", "sim_rf_scale_batch"):
        assert callable(getattr(mbfir, name))


@pytest.mark.parametrize("ntime,npoint,nscale", [
    ([1, 7, 255, 256, 257, 2000, 5000], [15, 256, 407, 256, 300, 300, 400], 4),
    ([300, 300, 10, 300], [1, 257, 512, 1000], 1),
    ([5], [100000], 3),
])
def test_block_table_covers_every_pulse_scale_and_chunk_once_longest_first(ntime, npoint, nscale):
    tab = mbfir.sim_block_table(ntime, npoint, nscale)
    chunks = [-(-n // 256) for n in npoint]
    assert tab.shape == (nscale * sum(chunks), 3)
    want = {(p, s, c) for p in range(len(ntime)) for s in range(nscale) for c in range(chunks[p])}
    got = [tuple(int(v) for v in row) for row in tab]
    assert len(set(got)) == len(got) and set(got) == want
    # pulses in descending order of ntime (ties in list order), each pulse's workgroups contiguous, scale-major within a pulse
    order = [int(p) for i, p in enumerate(tab[:, 0]) if i == 0 or tab[i - 1, 0] != p]
    assert order == sorted(range(len(ntime)), key=lambda p: (-ntime[p], p))
    for p in order:
        rows = tab[tab[:, 0] == p]
        assert [tuple(int(v) for v in r[1:]) for r in rows] == [(s, c) for s in range(nscale) for c in range(chunks[p])]


def test_block_table_rejects_bad_sizes():
    for nt, npt, ns in (([], [], 1), ([3], [0], 1), ([0], [5], 1), ([3], [5], 0), ([3, 4], [5], 1), ([3], [2 ** 62], 1)):
        with pytest.raises(ValueError):
            mbfir.sim_block_table(nt, npt, ns)


def _pulse(nt=8):
    return (np.full(nt, 0.01 + 0j), None, 4e-6, 1.0, 1.0, "C-13")


def test_python_argument_errors_come_before_any_device_work():
    df, dp = np.linspace(-100, 100, 5), 0.0
    with pytest.raises(ValueError, match="no pulses"):
        mbfir.bloch_batch([], df, dp)
    with pytest.raises(ValueError, match="scale list is empty"):
        mbfir.bloch_batch([_pulse()], df, dp, scales=[])
    with pytest.raises(ValueError, match="no samples"):
        mbfir.bloch_batch([_pulse(), _pulse(0)], df, dp)
    with pytest.raises(mbfir.MbfirError, match="Time-point length"):
        mbfir.bloch_batch([(np.ones(8), None, np.full(5, 4e-6), 1.0, 1.0, "C-13")], df, dp)
    with pytest.raises(ValueError, match="mode"):
        mbfir.bloch_batch([_pulse()], df, dp, mode=4)
    with pytest.raises(ValueError, match="empty grid"):
        mbfir.bloch_batch([_pulse(), _pulse()], [df, np.zeros(0)], dp)
    with pytest.raises(ValueError, match="no pulses"):
        mbfir.abr_batch([], df)
    with pytest.raises(ValueError, match="scale list is empty"):
        mbfir.abr_batch([np.ones(4)], df, scales=())
    with pytest.raises(ValueError, match="no samples"):
        mbfir.abr_batch([np.ones(4), np.zeros(0)], df)
    with pytest.raises(ValueError, match="one entry per rf sample"):
        mbfir.abr_batch([(np.ones(4), np.ones(3))], df)
    with pytest.raises(ValueError, match="convention"):
        mbfir.abr_batch([np.ones(4)], df, convention="abx")
    with pytest.raises(ValueError, match="nucleus"):
        mbfir.sim_rf_scale_batch([np.ones(4)], 0.01, nucleus="N-15", bw=1.0)
    with pytest.raises(ValueError, match="bw"):
        mbfir.sim_rf_scale_batch([np.ones(4), np.ones(4)], 0.01)
