"""CPU conditions on the integer-valued nets of tests/helpers/nn_exact.py, which
tests/test_gpu_nn_exact.py holds every network kernel to bit for bit.  No kernel is involved:
these are conditions on the chosen nets and inputs (density k, weight range, seed); a choice
that fails one is replaced by another, never given a tolerance.

Per case:
* every matmul site's input and weights equal their fp16 roundings, max |x| < 2048 and
  max sum |w x| < 2^24: no operand rounds and no f32 summation order matters;
* every policy logit is an integer;
* the net is not trivial: every 32-channel slice of every site's input has a nonzero entry,
  at least 10 % of each site's inputs are nonzero, at least a quarter of the policy logits
  (of the case's first 16 rows) take distinct values;
* the oracle's forward in modes 0 (fp32), 1 (fp16 emulation) and 2 (corrected emulation)
  gives the float64 policy with max |diff| == 0 -- exactness does not depend on one
  implementation's summation order -- and its value and misc logits stay within the a-priori
  f32 summation bound (nn_exact.head_bound; the ratio is printed);
* every mutation moves at least one policy logit (by >= 1, the logits being integers): a
  whole site, one tap, the tap transpose of a 3x3, one 32-input-channel slice, one
  16-output-channel tile, at every site (b18c384nbt: slices and tiles at the first, a middle
  and the last site of each kind).  vConv1 feeds the value head alone: its mutations must
  move a value or misc logit by more than twice that output's bound.  A mutation is looked
  for on two rows first (the first random position and a border board) and on the whole batch
  only if it does not show there; the sites before the mutated one are replayed, not
  recomputed.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("nn_exact", os.path.join(REPO, "tests", "helpers", "nn_exact.py"))
ex = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ex)

ORACLE_ROWS = 48  # the 1319-row batch goes through the oracle on its last rows only


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("exact_nets")


@pytest.mark.parametrize("name", list(ex.CASES))
def test_inputs_meet_the_exactness_conditions(model_dir, name):
    d = ex.case_data(name, model_dir, record=True)
    r, P = d["records"], d["P"]
    pol = d["R"][:, :P]
    print("%s: %d rows, %d sites, max |operand| %g, max sum |w x| %g, max |policy logit| %g, least nonzero share "
          "%.1f %%, emptiest slice %d channels lit, %d distinct of %d logits, max |value, misc| %.4g, forwards so far "
          "%d" % (name, len(pol), len(r), max(q["max_x"] for q in r), max(q["sum_abs"] for q in r), np.abs(pol).max(),
                  100 * min(q["nonzero"] for q in r), min(q["min_slice_channels"] for q in r),
                  len(np.unique(pol[:ex.DISTINCT_ROWS])), pol[:ex.DISTINCT_ROWS].size, np.abs(d["R"][:, P:]).max(),
                  ex.FORWARDS[0]))
    assert ex.conditions(r, d["R"], P, max_x=ex.CASES[name].get("max_x", 2048)) == []
    # the file holds the net: integers survive the float32 file exactly
    assert all(bool((p == p.round()).all()) for p in d["net"].parameters())


@pytest.mark.parametrize("name", list(ex.CASES))
def test_oracle_forward_is_exact_in_every_mode(model_dir, name):
    c = ex.CASES[name]
    d = ex.case_data(name, model_dir, record=True)
    P = d["P"]
    rows = slice(max(0, len(d["R"]) - ORACLE_ROWS), len(d["R"]))
    planes, glob, R, bound = d["planes"][rows], d["glob"][rows], d["R"][rows], d["bound"][rows]
    n = planes.shape[0]
    binp = np.ascontiguousarray(planes.reshape(n, -1, c["X"] * c["Y"]))
    model = oracle.Model(d["path"])
    for mode in (0, 1, 2):
        pol, val, misc = model.forward(c["X"], c["Y"], binp, glob, mode=mode, threads=4)
        diff = np.abs(pol.reshape(n, -1).astype(np.float64) - R[:, :P])
        head = np.abs(np.concatenate([val, misc], axis=1).astype(np.float64) - R[:, P:])
        print("%s mode %d: policy max |diff| %g; value and misc max |diff| %.3g on values up to %.4g, largest "
              "ratio to the bound %.3f (n = %d)" % (name, mode, diff.max(), head.max(), np.abs(R[:, P:]).max(),
                                                    (head[bound > 0] / bound[bound > 0]).max(), d["bound_n"]))
        assert diff.max() == 0, (mode, np.argwhere(diff != 0)[:5].tolist())
        if mode == 0:
            assert (head <= bound).all()


def test_shim_mutations_are_the_weight_mutations(model_dir):
    """Mutating a site's weights in the shim (with the earlier sites replayed) is forwarding a
    copy of the net with the mutated tensor."""
    name = "c80m48-5x5-padded"
    c = ex.CASES[name]
    d = ex.case_data(name, model_dir, record=True)
    sites = ex.f64.sites(d["net"], c["X"], c["Y"])
    _, base = ex.forward(d["net"], d["planes"], d["glob"], keep=True)
    i, sname = next((i, n) for i, n, kind, _ in sites if kind == "conv3" and n.startswith("blocks.0.inner.1"))
    for mutation in [("site",), ("tap", 5), ("slice", 1), ("tile", 2), ("transpose",)]:
        a, _ = ex.forward(d["net"], d["planes"], d["glob"], mutate=(i, mutation), replay=base.outputs)
        b, _ = ex.forward(ex.mutated(d["net"], sname, mutation), d["planes"], d["glob"])
        np.testing.assert_array_equal(a, b)
        assert not np.array_equal(a, d["R"])
    again, _ = ex.forward(d["net"], d["planes"], d["glob"])
    np.testing.assert_array_equal(again, d["R"])
    assert ex.train.F is torch.nn.functional and ex.train.torch is torch  # restored


def _moved(d, out, rows, label):
    """The mutation shows: a policy logit differs -- or, for vConv1, which feeds the value head
    alone, a value or misc logit moved by more than twice its bound, so that no output within
    the bound of the mutated net is within the bound of the true one."""
    P = d["P"]
    if label.startswith("vConv1."):
        return bool((np.abs(out[:, P:] - d["R"][rows, P:]) > 2 * d["bound"][rows]).any())
    return not np.array_equal(out[:, :P], d["R"][rows, :P])


@pytest.mark.parametrize("name", [n for n, c in ex.CASES.items() if c.get("mutate", True)])
def test_every_mutation_moves_a_policy_logit(model_dir, name):
    c = ex.CASES[name]
    d = ex.case_data(name, model_dir, record=True)
    P, n = d["P"], len(d["R"])
    quick = np.array([0, n - 1])  # a random position and a border board
    _, base = ex.forward(d["net"], d["planes"][quick], d["glob"][quick], keep=True)
    before = ex.FORWARDS[0]
    todo = ex.mutations(d["net"], c["X"], c["Y"], thin=c.get("thin", False))
    unseen, late = [], 0
    for (i, mutation), label in todo:
        out, _ = ex.forward(d["net"], d["planes"][quick], d["glob"][quick], mutate=(i, mutation), replay=base.outputs)
        if not _moved(d, out, quick, label):
            late += 1
            out, _ = ex.forward(d["net"], d["planes"], d["glob"], mutate=(i, mutation))
            if not _moved(d, out, slice(None), label):
                unseen.append(label)
    print("%s: %d mutations, %d needed the whole batch, %d forwards (%d so far in this process)" % (
        name, len(todo), late, ex.FORWARDS[0] - before, ex.FORWARDS[0]))
    print("%s: unseen %s" % (name, unseen))
    assert unseen == []
