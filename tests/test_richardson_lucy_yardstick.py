"""The yardstick of the Richardson-Lucy tests: the NumPy transcription of tests/helpers/rl_ref.py reproduces, bit for bit, the known
answers of tests/golden/rl_kat.json, which tests/golden/make_rl_kat.py computed with SciPy's own direct convolution."""
import json
import os

import numpy as np
import pytest

from helpers import rl_ref

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rl_kat.json")))


def kat_arrays(k):
    image = np.array(k["image"], np.float64).reshape(k["shape"])
    psf = np.array(k["psf"], np.float64).reshape(k["psf_shape"])
    want = np.array(k["want"], np.float64).reshape(k["shape"])
    return image, psf, want


def test_kat_holds_ranks_2_and_3_and_every_setting():
    assert {len(k["shape"]) for k in KAT} == {2, 3}
    assert {k["clip"] for k in KAT} == {True, False}
    assert {k["filter_epsilon"] for k in KAT} == {None, 1e-3, 0.2}
    assert any(0.0 in k["psf"] for k in KAT)
    assert any(max(k["want"]) == 1.0 for k in KAT if k["clip"]) and any(max(k["want"]) > 1.0 for k in KAT if not k["clip"])


@pytest.mark.parametrize("k", range(len(KAT)))
def test_transcription_reproduces_the_known_answers_bit_for_bit(k):
    image, psf, want = kat_arrays(KAT[k])
    got = rl_ref.richardson_lucy(image, psf, KAT[k]["iterations"], KAT[k]["clip"], KAT[k]["filter_epsilon"])
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), int((got.view(np.uint64) != want.view(np.uint64)).sum())
