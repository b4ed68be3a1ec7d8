"""The fused network's logits, bit for bit, against a recording of an earlier build
(tests/golden/nn_fused_bits.npz, written by tools/record_nn_bits.py): changes to the
kernel's non-arithmetic parts -- load scheduling, staging, which lanes run which linear --
must not move a single bit of any instance's output.

Cases (tools/record_nn_bits.py holds the inputs): b6c96 @ 5x5, two random-init models;
fast / accurate / corrected at 1, 5, 6 and 13 boards (full outputs); fast at
5 x CUs + 1 boards, the smallest batch on the 8-board instance (SHA-256; the recording
holds the CU count it was made at); and a 12-game, 96-round self-play on
the fast network, which reaches the kernel through the device-side count and row index
(SHA-256 of the drained row arrays and of the games' search trees).
"""
import importlib.util
import os

import numpy as np
import pytest

import katacoffee_amd as kc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_nn_bits", os.path.join(REPO, "tools", "record_nn_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def gold():
    with np.load(rec.GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def model_paths(tmp_path_factory):
    return rec.write_models(kc, str(tmp_path_factory.mktemp("bits_nets")))


@pytest.mark.parametrize("mi", range(len(rec.MODEL_SEEDS)))
def test_small_batches_bit_identical(gold, model_paths, mi):
    got = rec.small_outputs(kc, model_paths[mi], mi)
    assert len(got) == len(rec.PRECISIONS) * len(rec.SIZES)
    for key, o in got.items():
        want = gold[key]
        assert o.shape == want.shape and o.dtype == want.dtype, key
        assert np.isfinite(o).all(), key
        diff = np.flatnonzero(o.view(np.uint32).ravel() != want.view(np.uint32).ravel())
        assert diff.size == 0, "%s: %d of %d outputs differ in bits (first at flat index %d)" % (
            key, diff.size, o.size, diff[0])


@pytest.mark.parametrize("mi", range(len(rec.MODEL_SEEDS)))
def test_eight_board_instance_bit_identical(gold, model_paths, mi):
    cus = rec.cu_count()
    assert cus == int(gold["cus"]), "recorded on a %d-CU device (MI355X), this one has %d: re-record" % (
        int(gold["cus"]), cus)
    assert rec.big_hash(kc, model_paths[mi], mi, cus) == str(gold["m%d_fast_big_sha" % mi])


@pytest.mark.parametrize("mi", range(len(rec.MODEL_SEEDS)))
def test_selfplay_count_and_row_index_path_bit_identical(gold, model_paths, mi):
    for name, hx in rec.selfplay_hashes(kc, model_paths[mi], mi):
        assert hx == str(gold["m%d_sp_%s" % (mi, name)]), "self-play %s differs from the recording" % name
