"""CPU checks of the float64 reference and its operand-loss probes (tests/helpers/nn_f64.py),
which tests/test_gpu_nn_split.py holds the accurate kernels against:

* wrapping train's matmul sites changes nothing while no probe is selected;
* the float64 reference is the network the oracle's fp32 forward computes (2e-4, the bound
  test_train.py holds torch against the oracle with);
* rounding every site on both sides gives what the oracle's fp16-emulation mode 1 gives,
  within that mode's bound 2e-3 x max(1, max |logit|): the probes round where the fp16
  kernels round;
* on every shared case each retained probe moves the logits, and the smallest signature is
  at least 8 x the float32 forward's own distance from float64 -- a condition on the chosen
  nets and inputs (seed, scale), not a measurement of any kernel.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from katacoffee_amd import train
from oracle import oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("nn_f64", os.path.join(REPO, "tests", "helpers", "nn_f64.py"))
f64 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(f64)

ALL = [(name, False) for name in f64.CASES] + [(name, True) for name in f64.RANDOM_INIT]
IDS = ["%s%s" % (n, "-rand" if r else "") for n, r in ALL]


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("f64_nets")


def _oracle(path, c, d, mode):
    n = d["planes"].shape[0]
    binp = np.ascontiguousarray(d["planes"].reshape(n, -1, c["X"] * c["Y"]))
    pol, val, misc = oracle.Model(path).forward(c["X"], c["Y"], binp, d["glob"], mode=mode, threads=4)
    return np.concatenate([pol.reshape(n, -1), val, misc], axis=1)


def test_wrapping_without_a_probe_changes_nothing():
    net = f64.make_net("b2c32nbt", 5).double()
    planes, glob = f64.boards(6, 5, 5, 4, seed=5)
    b, g = torch.from_numpy(planes).double(), torch.from_numpy(glob).double()
    with torch.no_grad():
        plain = torch.cat(net(b, g), dim=1).numpy()
        with f64.probing() as p:
            wrapped = torch.cat(net(b, g), dim=1).numpy()
        again = torch.cat(net(b, g), dim=1).numpy()
    np.testing.assert_array_equal(wrapped, plain)
    np.testing.assert_array_equal(again, plain)
    assert train.F is torch.nn.functional and train.torch is torch  # restored
    # kinds [3, 2]: stem, (convP, conv1, conv1g, conv2, conv1, conv2, convQ), (convP, 2 x (conv1, conv2), convQ),
    # pConv1, pConvG, pConv2, vConv1 -- numbered in call order
    assert [s[0] for s in p.sites] == list(range(18))
    names = [s[1] for s in f64.sites(net, 5, 5)]
    assert names[0] == "convInit" and names[1] == "blocks.0.convP" and names[-4:] == ["pConv1", "pConvG", "pConv2",
                                                                                     "vConv1"]
    # a probe moves the result, and only for the duration of its context
    R, sig, e32 = f64.signatures(net, planes, glob, [(1, "w", ("all",)), (1, "x", ("slice", 1))])
    np.testing.assert_array_equal(R, plain)
    assert (sig > 0).all() and e32 > 0


def test_partial_probes_add_up_to_the_whole_site():
    """Rounding every tap (or every slice) of a site's operand is rounding the whole operand."""
    net = f64.make_net(dict(C=64, Cg=16, p1=32, g1=32, v1=32, v2=64, kinds=[0]), 3).double()
    planes, glob = f64.boards(4, 5, 5, 4, seed=1)
    for operand in ("w", "x"):
        whole = f64._forward(net, planes, glob, [(1, operand, ("all",))])[0]
        taps = f64._forward(net, planes, glob, [(1, operand, ("tap", t)) for t in range(9)])[0]
        slices = f64._forward(net, planes, glob, [(1, operand, ("slice", j)) for j in range(2)])[0]
        np.testing.assert_allclose(taps, whole, rtol=0, atol=1e-12)
        np.testing.assert_allclose(slices, whole, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name,rand", ALL, ids=IDS)
def test_reference_vs_oracle_and_signatures(model_dir, name, rand):
    c = f64.CASES[name]
    d = f64.case_data(name, model_dir, rand)
    R, sig, e32 = d["R"], d["sig"], d["e32"]
    top = float(np.abs(R).max())
    # float64 reference vs the oracle's fp32 forward
    e_ora = float(np.abs(_oracle(d["path"], c, d, 0) - R).max())
    # every site rounded on both sides vs the oracle's fp16 emulation
    r16 = f64._forward(d["net"], d["planes"], d["glob"], f64.both_sides(d["net"], c["X"], c["Y"]))[0]
    e_16 = float(np.abs(_oracle(d["path"], c, d, 1) - r16).max())
    k = int(sig.argmin())
    print("%s: %d probes, max |logit| %.3g, oracle fp32 vs R %.3g, fp16 emulation vs both-sides %.3g, "
          "e32 %.3g, sigma_min %.3g (%s), ratio %.1f" % (name, len(sig), top, e_ora, e_16, e32, sig[k], d["labels"][k],
                                                         sig[k] / e32))
    assert e_ora <= 2e-4
    assert e_16 <= 2e-3 * max(1.0, top)
    assert (sig > 0).all(), [d["labels"][i] for i in np.flatnonzero(sig <= 0)]
    assert sig[k] >= 8 * e32
    assert len(sig) <= 170  # the probe list stays small
