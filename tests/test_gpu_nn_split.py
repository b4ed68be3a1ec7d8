"""Every split-precision ("accurate") instance against a float64 reference, with a bound
that a single lost cross term would break.

The accurate kernels form each product as hi(w) hi(x) + lo(w) hi(x) + hi(w) lo(x) on three
MFMAs.  tests/helpers/nn_f64.py computes, in float64 on the CPU, the reference R and for a
list of probes what the logits would be had the second or the third product gone missing at
one convolution -- or at one tap, or one 32-channel K slice of it.  sigma_min is the smallest
of those displacements max |R_probe - R| over the case's probes.

Per case:
  e_dev  = max |accurate instance - R|  <=  sigma_min / 2
  e_fast = max |fp16 instance - R|      >   sigma_min / 2     (the control)
The factor is derived, not measured: an instance that lost a probed term ends at least
sigma - e_legit from R, so the bound catches the loss whenever the legitimate error is
below sigma / 2, and passes a correct kernel under the same condition.  The control shows
the bound fails a kernel without the cross terms.  (tests/test_nn_f64_reference.py holds
sigma_min >= 8 x the float32 forward's own error e32 on every case, on the CPU.)

Cases (helpers/nn_f64.py CASES; batches ragged against the instance's boards per workgroup):
  b6c96 @ 5x5             fused SPLIT3 borderless 5-board instance, 7 rows; per tap and slice
                          on block 0's convs and a gpool block
  b6c96 @ 5x5 nb2         the 2-board bordered instance, 3 rows
  b6c96 @ 7x7             layered, C = 96 -> tn 3, gpool conv2 with 64 inputs
  C=64 [0] @ 5x5          layered tn 2, per tap and slice on every site
  C=96 Cg=32 [1] @ 7x7    layered tn 3, PRO_BN_GB, merged conv1 + conv1g
  C=128 [0] @ 9x9         layered tn 4
  C=384 mid=192 [3,2] @ 9x9   split kConv1L at 384 and 192 inputs, 192-wide 3x3
  C=80 mid=48 Cg=24 [3] @ 5x5 padded K slices and output tiles
  b10c128 @ 7x7 default   what the C4 line runs
  limits @ 5x5            p1 = g1 = 64, v1 = 128, v2 = 256, Cg = 128 together (C = 160)
  C=68 mid=36 odd heads   the granularity the layered kernels take (multiples of 4; head and
                          gpool widths free)
and for the named architectures the engine's own random-init net as well.

Excluded probes (no rounded operand exists there): the stem's activation side (0/1 planes,
exact in fp16) and pConv2 (f32 outside the MFMAs).

Then the widths NNLayered refuses: one past each limit, a trunk or bottleneck width that is
not a multiple of 4, a net too wide for the LDS at its board size -- creation fails, nothing
is launched, the library works afterwards.
"""
import importlib.util
import os

import numpy as np
import pytest

import katacoffee_amd as kc
from katacoffee_amd import train

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("nn_f64", os.path.join(REPO, "tests", "helpers", "nn_f64.py"))
f64 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(f64)

ALL = [(name, False) for name in f64.CASES] + [(name, True) for name in f64.RANDOM_INIT]
IDS = ["%s%s" % (n, "-rand" if r else "") for n, r in ALL]


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("split_nets")


def _device(path, c, packed, precision):
    net = kc.Network(path, c["X"], c["Y"], c["W"], precision=precision)
    fused = net.fused
    out = net.forward(packed)
    net.close()
    assert np.isfinite(out).all(), precision
    return out.astype(np.float64), fused


@pytest.mark.parametrize("name,rand", ALL, ids=IDS)
def test_accurate_instance_within_half_the_smallest_signature(model_dir, name, rand):
    c = f64.CASES[name]
    d = f64.case_data(name, model_dir, rand)
    R, sig, e32 = d["R"], d["sig"], d["e32"]
    k = int(sig.argmin())
    bound = sig[k] / 2
    packed = f64.pack_u64(d["planes"])
    layered = c["fast"] == "fast-layered"
    results = []
    for precision in c["accurate"]:
        out, fused = _device(d["path"], c, packed, precision)
        assert fused == (not layered)
        results.append((precision, float(np.abs(out - R).max())))
    out, _ = _device(d["path"], c, packed, c["fast"])
    e_fast = float(np.abs(out - R).max())
    for precision, e_dev in results:
        print("%s%s %s: e_dev %.3g e32 %.3g sigma_min %.3g (%s) e_dev/sigma_min %.3f | %s e_fast %.3g | max |logit| "
              "%.3g, %d probes" % (name, "-rand" if rand else "", precision, e_dev, e32, sig[k], d["labels"][k],
                                   e_dev / sig[k], c["fast"], e_fast, np.abs(R).max(), len(sig)))
    for precision, e_dev in results:
        assert e_dev <= bound, (precision, e_dev, bound, d["labels"][k])
    assert e_fast > bound, (c["fast"], e_fast, bound)


# -- widths ------------------------------------------------------------------------------
LIMITS = f64.CASES["limits-5x5"]["cfg"]
GRAIN = f64.CASES["c68m36-5x5-odd"]["cfg"]
BOTH = ("accurate", "fast-layered", "default")
REFUSED = [
    # one past each of the constructor's limits in turn
    ("p1", dict(LIMITS, p1=65), "p1", BOTH),
    ("g1", dict(LIMITS, g1=65), "g1", BOTH),
    ("v1", dict(LIMITS, v1=129), "v1", BOTH),
    ("v2", dict(LIMITS, v2=257), "v2", BOTH),
    ("Cg", dict(LIMITS, Cg=129), "Cg", BOTH),
    ("input-planes", dict(LIMITS, cin=33), "input planes", BOTH),
    ("global-inputs", dict(LIMITS, gin=2), "global inputs", BOTH),
    # the granularity: C = 68 and mid = 36 run (the case above), 66 and 34 do not
    ("C-not-multiple-of-4", dict(GRAIN, C=66), "multiple of 4", BOTH),
    ("mid-not-multiple-of-4", dict(GRAIN, mid=34), "multiple of 4", BOTH),
    # the LDS budget: a gpool block's conv2 keeps a [boards][C - Cg] bias beside its stages, and the
    # split kernel's four stages of ten 5x5 boards leave 7040 bytes: 12 C - 10 Cg <= 1760 (C = 160,
    # Cg = 128 above passes with 640; b10c128 with 1216); C = 192, Cg = 32 needs 1984
    ("too-wide-for-LDS", dict(C=192, Cg=32, p1=32, g1=32, v1=32, v2=64, kinds=[1]), "LDS", ("accurate", "default")),
]


@pytest.mark.parametrize("what,cfg,word,precisions", REFUSED, ids=[r[0] for r in REFUSED])
def test_unsupported_widths_are_refused_at_creation(model_dir, what, cfg, word, precisions):
    path = os.path.join(str(model_dir), "refused-%s.cfnn" % what)
    cfg = dict(cfg)
    net = train.CoffeeNet(cfg, cin=cfg.pop("cin", train.NUM_SPATIAL), gin=cfg.pop("gin", 1))
    train.save_cfnn(net, path)
    assert kc.model_flops(path, 25) > 0  # the loader takes the file: the refusal is NNLayered's
    for precision in precisions:
        with pytest.raises(kc.CoffeeError) as ei:
            kc.Network(path, 5, 5, 4, precision=precision)
        assert word in str(ei.value) and "NNLayered" in str(ei.value), str(ei.value)
    # and the library still works afterwards
    good = f64.case_data("c64-5x5-tn2", model_dir)
    net = kc.Network(good["path"], 5, 5, 4, precision="accurate")
    out = net.forward(f64.pack_u64(good["planes"]))
    net.close()
    assert float(np.abs(out - good["R"]).max()) <= good["sig"].min() / 2
