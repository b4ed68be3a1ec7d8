"""Uncertainty weighting of playouts, the checks that need no GPU: the host
run of the weight formula against a float64 restatement, the commands' config keys, and the
trainer's short-term error loss."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import katacoffee_amd as kc
from katacoffee_amd import train
from oracle import oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(kc.LIB_PATH):
        kc.build()
    return kc.lib()


# ---------------------------------------------------------------------------------------
# 1. coffee_uncertainty_weight against float64.

# Largest relative difference of the f32 weight (polynomial dexp / dlog / dpow chain) from the
# float64 restatement below over GRID x CASES, measured with this file's _measure(): 4.762e-03
# (exponent 0.5, coefficient 0.05, logit -30).  It is not the polynomials: below a logit of
# about -24 the f32 sum 1 + exp(0.5 x) keeps only a few bits of exp(0.5 x), so the error (of the
# order 1e-7 there) is off by up to half of itself, and an exponent below 1 lifts that into
# sight of the floor coeff / max_weight.  From logit -16 up the largest difference is 3.8e-05;
# at exponent 1 it is 4.8e-06 over the whole grid.  The test asserts at four times the measured
# figure.
MEASURED_REL = 4.762e-03
TOL = 4.0 * MEASURED_REL
GRID = np.arange(-30.0, 100.0 + 1e-9, 0.25)  # 0.5 x > 40 from logit 80.25 on
CASES = [(e, c) for e in (1.0, 0.5, 0.7) for c in (0.25, 0.05)]
MAX_W = 8.0


def _ref(logit, coeff, exponent, max_weight):
    h = 0.5 * float(logit)
    s = h if h > 40.0 else math.log1p(math.exp(h))
    err = math.sqrt(s * s * 0.25)
    return err, coeff / (err ** exponent + coeff / max_weight)


def _measure(L):
    worst = (0.0, None)
    worst_err = 0.0
    for e, c in CASES:
        for x in GRID:
            x = float(np.float32(x))
            err, w = kc.uncertainty_weight(x, use_uncertainty=1, uncertainty_coeff=c, uncertainty_exponent=e,
                                           uncertainty_max_weight=MAX_W)
            # the parameters as the library holds them (f32)
            rerr, rw = _ref(x, float(np.float32(c)), float(np.float32(e)), MAX_W)
            rel = abs(float(w) - rw) / rw
            if rel > worst[0]:
                worst = (rel, (e, c, x))
            worst_err = max(worst_err, abs(float(err) - rerr) / max(rerr, 1.0))
    return worst, worst_err


def test_weight_matches_float64(L):
    (rel, where), err_dev = _measure(L)
    print("largest relative weight difference %.3e at (exponent, coeff, logit) %s; err %.3e" % (rel, where, err_dev))
    assert rel <= TOL, (rel, where)
    # the error itself, on the scale max(err, 1): 1 + exp(h) rounds to f32 before the log (an
    # absolute 2^-24 = 6e-8 in s where s is small) and the chain is about ten f32 operations of
    # relative 6e-8 each elsewhere, so 1e-6 bounds it
    assert err_dev <= 1e-6
    assert float(GRID[-1]) * 0.5 > 40.0 > float(GRID[0]) * 0.5  # both branches of s are on the grid


def test_weight_is_monotone_and_saturates(L):
    for e, c in CASES:
        w = [float(kc.uncertainty_weight(float(x), use_uncertainty=1, uncertainty_coeff=c, uncertainty_exponent=e,
                                         uncertainty_max_weight=MAX_W)[1]) for x in GRID]
        assert all(a >= b for a, b in zip(w, w[1:])), (e, c)
        assert w[0] > w[-1] > 0.0
        # logit -> -inf: err -> 0, w -> max_weight
        for x in (-200.0, -1e30, -math.inf):
            err, wm = kc.uncertainty_weight(x, use_uncertainty=1, uncertainty_coeff=c, uncertainty_exponent=e,
                                            uncertainty_max_weight=MAX_W)
            assert err == 0.0 and abs(float(wm) - MAX_W) <= TOL * MAX_W, (e, c, x, wm)
    # off: every weight is 1, the error is still reported
    err, w = kc.uncertainty_weight(0.5)
    assert w == 1.0 and err > 0.0


@pytest.mark.parametrize("field,value", [("uncertainty_coeff", 0.0), ("uncertainty_coeff", 1.5),
                                         ("uncertainty_coeff", math.nan), ("uncertainty_exponent", -0.1),
                                         ("uncertainty_exponent", 2.5), ("uncertainty_exponent", math.inf),
                                         ("uncertainty_max_weight", 0.5), ("uncertainty_max_weight", 101.0),
                                         ("uncertainty_max_weight", math.nan), ("use_uncertainty", 2)])
def test_bad_parameters_are_rejected(L, field, value):
    p = kc.default_uncertainty_params(use_uncertainty=1)
    setattr(p, field, value)
    err, w = ctypes.c_float(), ctypes.c_float()
    rc = L.coffee_uncertainty_weight(ctypes.byref(p), ctypes.c_float(0.0), ctypes.byref(err), ctypes.byref(w))
    assert rc == -1 and field in L.coffee_last_error().decode()  # COFFEE_EINVAL
    with pytest.raises(kc.CoffeeError, match=field):
        kc.uncertainty_weight(0.0, p)


def test_defaults(L):
    p = kc.default_uncertainty_params()
    # off; gatekeeper1.cfg:108-110 / setup.cpp:539-562 values
    assert p.use_uncertainty == 0 and p.uncertainty_coeff == 0.25 and p.uncertainty_exponent == 1.0
    assert p.uncertainty_max_weight == 8.0
    assert L.coffee_abi_version() == 108
    assert ctypes.sizeof(kc.UncertaintyParams) == 16


# ---------------------------------------------------------------------------------------
# 2. Config keys (cli_config.h, shared by katago selfplay / gatekeeper / analysis).

@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("unc") / "unc_config_dump")
    if not os.path.exists(kc.LIB_PATH):
        kc.build()
    libdir = os.path.dirname(kc.LIB_PATH)  # linked as the katago program is (csrc/Makefile)
    subprocess.run(["g++", "-std=c++17", "-O0", "-o", exe, os.path.join(REPO, "tests", "helpers", "unc_config_dump.cpp"),
                    "-L" + libdir, "-lkatacoffee", "-Wl,-rpath," + libdir], check=True)

    def run(text, tmp_path):
        cfg = tmp_path / "c.cfg"
        cfg.write_text(text)
        r = subprocess.run([exe, str(cfg)], capture_output=True, text=True, timeout=30)
        return r.returncode, r.stdout.split(), r.stderr
    return run


def test_config_keys_reach_the_params(dump, tmp_path):
    rc, out, _ = dump("maxVisits = 100\nuseUncertainty = true\nuncertaintyCoeff = 0.5\n"
                      "uncertaintyExponent = 0.5  # a comment\nuncertaintyMaxWeight = 4\n", tmp_path)
    assert rc == 0 and [int(out[0])] + [float(x) for x in out[1:]] == [1, 0.5, 0.5, 4.0]
    # the reference's own lines (gatekeeper1.cfg:108-110)
    rc, out, _ = dump("useUncertainty = true\nuncertaintyExponent = 1.0\nuncertaintyCoeff = 0.25\n", tmp_path)
    assert rc == 0 and [int(out[0])] + [float(x) for x in out[1:]] == [1, 0.25, 1.0, 8.0]


def test_absent_config_keys_mean_off(dump, tmp_path, L):
    rc, out, _ = dump("maxVisits = 100\n# useUncertainty = true\n", tmp_path)
    d = kc.default_uncertainty_params()
    assert rc == 0 and int(out[0]) == 0 == d.use_uncertainty
    assert [float(x) for x in out[1:]] == [d.uncertainty_coeff, d.uncertainty_exponent, d.uncertainty_max_weight]
    rc, out, _ = dump("useUncertainty = false\n", tmp_path)
    assert rc == 0 and int(out[0]) == 0


@pytest.mark.parametrize("key,value", [("uncertaintyCoeff", "0.00001"), ("uncertaintyCoeff", "1.5"),
                                       ("uncertaintyExponent", "-1"), ("uncertaintyExponent", "2.01"),
                                       ("uncertaintyMaxWeight", "0.9"), ("uncertaintyMaxWeight", "1000"),
                                       ("uncertaintyMaxWeight", "nan"), ("uncertaintyCoeff", "0.25x")])
def test_out_of_range_config_values_are_rejected(dump, tmp_path, key, value):
    rc, out, err = dump("useUncertainty = true\n%s = %s\n" % (key, value), tmp_path)
    assert rc == 1 and key in err and not out, (rc, out, err)


def test_shipped_configs_keep_the_setting_off():
    """The shipped configs may name the keys in comments only."""
    cfgdir = os.path.join(REPO, "configs")
    for name in sorted(os.listdir(cfgdir)):
        for line in open(os.path.join(cfgdir, name)):
            code = line.split("#", 1)[0]
            assert "ncertainty" not in code, (name, line)


# ---------------------------------------------------------------------------------------
# 3. Trainer: the short-term error loss.

@pytest.fixture(scope="module")
def batch():
    sp = oracle.Selfplay(5, 5, 4, games=2, max_visits=12, node_cap=64)
    sp.rounds(600)
    rows = sp.rows()
    assert len(rows["meta"]) >= 16
    b = train.rows_to_batch(rows, 5, 5)
    gt = rows["globalTargetsNC"]
    # the key is win - loss of the pair written with now-factor 1 / (1 + 0.016 A): not the final
    # outcome (pair 0) and inside [-1, 1]
    np.testing.assert_array_equal(b["v_short"].numpy(), gt[:, 6] - gt[:, 7])
    assert np.all(np.abs(b["v_short"].numpy()) <= 1.0)
    assert np.any(gt[:, 6] != gt[:, 0]) and np.any(gt[:, 6] != gt[:, 4])
    return b


def _net(seed=0):
    torch.manual_seed(seed)
    net = train.CoffeeNet("b2c32")
    with torch.no_grad():  # a random net's error head, not the zero bias alone
        net.vBM.copy_(torch.tensor([0.3, -0.2]))
    return net


def test_st_error_loss_trains_the_error_head_only(batch):
    net = _net()
    policy, value, misc = net(batch["binp"], batch["glob"])
    value.retain_grad()
    policy.retain_grad()
    loss = train.st_error_loss(value, misc, batch["v_short"])
    # the restated formula, in float64
    p = torch.softmax(value.detach().double(), dim=1)
    pred = 0.25 * torch.nn.functional.softplus(0.5 * misc.detach().double()[:, 1]) ** 2
    tgt = (p[:, 0] - p[:, 1] - batch["v_short"].double()) ** 2 + 1e-8
    d = (pred - tgt).abs()
    want = 2.0 * torch.where(d < 0.4, 0.5 * d * d, 0.4 * (d - 0.2)).mean()
    assert float(loss.detach()) == pytest.approx(float(want), rel=1e-5)
    loss.backward()
    # nothing flows through the value head's output (the prediction is detached) or the policy
    assert value.grad is None or torch.all(value.grad == 0)
    assert policy.grad is None or torch.all(policy.grad == 0)
    for p in (net.vLin3, net.vB3, net.pConv2, net.pLinG):
        assert p.grad is None or torch.all(p.grad == 0)
    # of the misc head, only row 1 (the short-term error logit); row 0 (variance time) stays untrained
    assert torch.all(net.vLinM.grad[0] == 0) and net.vBM.grad[0] == 0
    assert torch.any(net.vLinM.grad[1] != 0) and net.vBM.grad[1] != 0


def test_st_error_loss_falls_under_adam(batch):
    net = _net(1)
    opt = torch.optim.Adam(net.parameters(), lr=2e-3)

    def cur():
        with torch.no_grad():
            _, value, misc = net(batch["binp"], batch["glob"])
            return float(train.st_error_loss(value, misc, batch["v_short"]))
    before = cur()
    for _ in range(30):
        pl, vl = train.train_step(net, opt, batch, st_error_weight=1.0)
    assert math.isfinite(pl) and math.isfinite(vl)
    assert cur() < before


def test_zero_st_error_weight_is_todays_step(batch):
    nets = [_net(2) for _ in range(3)]
    opts = [torch.optim.Adam(n.parameters(), lr=2e-3) for n in nets]
    for _ in range(3):
        train.train_step(nets[0], opts[0], batch)                       # the unchanged call
        train.train_step(nets[1], opts[1], batch, st_error_weight=0.0)
        # the step as it was before the term existed
        opts[2].zero_grad()
        pl, vl = train.losses(nets[2], batch)
        (pl + 1.0 * vl).backward()
        opts[2].step()
    for a, b, c in zip(nets[0].tensors(), nets[1].tensors(), nets[2].tensors()):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert len(train.losses(nets[0], batch)) == 2
    # and the term does change the step when it is on
    train.train_step(nets[0], opts[0], batch)
    train.train_step(nets[1], opts[1], batch, st_error_weight=1.0)
    assert not torch.equal(nets[0].vLinM, nets[1].vLinM)
