"""The emulation edition of the primitives (rapmap_amd/csrc/qm_wave.h under -DQM_EMU, and key_count of qm_selpack.inl) against a numpy
restatement of what the comment above each primitive promises (tests/wave_cases.py), bit for bit, one test id per primitive (and per value
of its wave-uniform parameter).  The CPU suite checks the wave bodies lane by lane on these definitions; test_wave_primitives_gpu.py holds
the device edition to them."""
import numpy as np
import pytest

import wave_cases as wc


@pytest.fixture(scope="module")
def emu():
    import emu_wave
    emu_wave._lib()
    return emu_wave


def test_every_op_of_the_probe_has_a_case(emu):
    assert emu.sizes() == (wc.MEMB, wc.NOUT)
    assert set(emu.ops()) == {k.op for k in wc.CASES.values()} == set(wc.EXPECT)


def test_launch_shape_of_the_cases():
    """at least two blocks of four wavefronts per case, a few hundred wavefronts at the most"""
    for k in wc.CASES.values():
        assert 8 <= k.w <= 400, (k.name, k.w)


@pytest.mark.parametrize("name", wc.NAMES)
def test_emulation_edition(emu, name):
    k = wc.CASES[name]
    out, _ = wc.check(emu.wave, name)
    if k.op == "group_sum_f64":                                           # every lane of a group ends with the same bits
        assert wc.same_bits_in_a_group(out, int(k.prm[0])), name
    elif k.op == "wave_sum_f64":
        assert wc.same_bits_in_a_group(out, 64), name
    elif k.op == "quarters_sum_f64":                                      # the four lanes of a column l % 16
        x = out[:, 0, :].reshape(-1, 4, 16)
        assert (x == x[:, :1, :]).all(), name


def test_the_restatement_can_fail(emu):
    """the comparison is on every lane and every bit: one flipped bit of one lane's input shows"""
    k = wc.CASES["row8_or"]
    a = k.a.copy(); a[3, 17] ^= np.uint64(1 << 9)
    out, _ = emu.wave(k.op, k.prm, a, k.b, k.c, k.d, k.mem, k.atom)
    want, _ = k.want()
    assert (out[:, 0, :] != want[0]).sum() == 8                           # the eight lanes of that row of the tile
