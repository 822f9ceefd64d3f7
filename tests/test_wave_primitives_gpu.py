"""The device edition of the primitives (rapmap_amd/csrc/qm_wave.h as the product compiles it for gfx950 -- DPP control words and row masks,
ds_bpermute addresses from threadIdx.x, v_perm_b32, packed 16-bit arithmetic, global_load_lds, scalar loads, doubles as two dwords -- and
key_count's carry chain in qm_selpack.inl) against the emulation edition and against the numpy restatement (tests/wave_cases.py), bit for
bit, one test id per primitive.  Both editions run one probe body (tests/device/qm_wave_probe.inl); on the device a case is ONE launch of
blocks of four wavefronts, a wave of the case per wavefront, so the lane addresses built from threadIdx.x are exercised in wavefronts 1 .. 3
of a block as well."""
import os
import sys

import numpy as np
import pytest

import wave_cases as wc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "device"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(lib_built):                                                       # (torch opens the device before the probe's runtime does)
    import probe
    probe._lib()
    return probe


@pytest.fixture(scope="module")
def emu():
    import emu_wave
    emu_wave._lib()
    return emu_wave


def test_both_editions_run_the_same_probe(dev, emu):
    assert dev.ops() == emu.ops()
    assert (dev._lib().qp_memb(), dev._lib().qp_nout()) == emu.sizes() == (wc.MEMB, wc.NOUT)


@pytest.mark.parametrize("name", wc.NAMES)
def test_device_edition(dev, emu, name):
    k = wc.CASES[name]
    before = dev.launches
    out, atom = wc.check(dev.wave, name)                                  # ... against the restatement
    assert dev.launches == before + 1
    eout, eatom = emu.wave(k.op, *k.args())                               # ... and against the emulation edition
    bad = np.argwhere(out != eout)
    assert not len(bad), "%s: device and emulation differ in %d places, first at wave %d (wavefront %d of its block) row %d lane %d: %#x / %#x" % (
        name, len(bad), bad[0][0], bad[0][0] % 4, bad[0][1], bad[0][2], int(out[tuple(bad[0])]), int(eout[tuple(bad[0])]))
    assert np.array_equal(atom, eatom), name
    if k.op == "group_sum_f64":
        assert wc.same_bits_in_a_group(out, int(k.prm[0])), name
    elif k.op == "wave_sum_f64":
        assert wc.same_bits_in_a_group(out, 64), name
    elif k.op == "quarters_sum_f64":
        x = out[:, 0, :].reshape(-1, 4, 16)
        assert (x == x[:, :1, :]).all(), name
