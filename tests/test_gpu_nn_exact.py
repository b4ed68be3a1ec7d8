"""Every network kernel, bit for bit, against float64 on integer-valued nets.

tests/helpers/nn_exact.py builds nets with small integer weights, unit norm scales and integer
biases whose every matmul operand is an integer below 2048 (exact in fp16: lo = 0 in the split
and the corrected schemes) and whose every sum of |w x| is below 2^24 (any f32 summation order
is exact); tests/test_nn_exact_reference.py asserts those conditions on the CPU, and that every
site, tap, 32-channel K slice and 16-channel output tile of the net moves a policy logit.  Such
a net has one possible policy output.  Per case and per precision (fast, fast-layered,
accurate, corrected, default; accurate-nb2 for b6c96 @ 5x5)

  np.array_equal(out[:, :4A], R_policy.astype(np.float32))

with R the float64 forward of train.CoffeeNet.  The value head pools means (S / A is not exact),
so value and misc are held to the a-priori f32 summation bound n 2^-24 S per output
(nn_exact.head_bound: S the head's linears on absolute values, n the longest dot product plus
4); the largest ratio to the bound is printed.

Cases: nn_f64's geometries, configs and batches (ragged against the boards per workgroup) plus
two border-only boards each; b6c96 @ 5x5 also on 5 x 256 + 39 rows (the fused 8-board
instance), on the last 203 of them (the 5-board instance) and on the last row alone, and with
a net whose operands stay within e4m3's 448 (on the others the corrected instance flags every
board and what is compared is the split re-evaluation; on this one default resolves to
corrected and the e4m3 MFMAs' own output is compared); b2c32nbt @ 5x5; b18c384nbt @ 9x9.  Then
forward_canonical on a fused and a layered net, the self-play batch protocol (device-side
count and row indirection) on the b6c96 net, and a control: one tap of one mid-trunk 3x3
zeroed in the file, which the comparison must see.
"""
import importlib.util
import os

import numpy as np
import pytest

import katacoffee_amd as kc
from katacoffee_amd import train
from oracle import oracle

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _helper(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "tests", "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ex = _helper("nn_exact")
symmetry = _helper("symmetry")
pack_u64 = ex.f64.pack_u64

PRECISIONS = ("fast", "fast-layered", "accurate", "corrected", "default")
COMBOS = [(name, p) for name in ex.CASES for p in PRECISIONS] + [("b6c96-5x5", "accurate-nb2"),
                                                                  ("b6c96-5x5-nb2", "accurate-nb2")]


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("exact_nets")


def _network(path, c, precision):
    try:
        return kc.Network(path, c["X"], c["Y"], c["W"], precision=precision)
    except kc.CoffeeError as e:
        if "NNLayered" not in str(e):
            raise
        pytest.skip("the constructor refuses %s for this net: %s" % (precision, e))


def _check(tag, out, R, bound, P, A, fused):
    """Policy bit-equal to the reference; value and misc within their bound."""
    want = R[:, :P].astype(np.float32)
    got = out[:, :P]
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        row, k = (int(v) for v in bad[0])
        print("%s: %d of %d policy logits differ; first at row %d direction %d cell %d: device %r reference %r; "
              "net.fused %s" % (tag, len(bad), got.size, row, k // A, k % A, float(got[row, k]), float(want[row, k]),
                                fused))
    head = np.abs(out[:, P:].astype(np.float64) - R[:, P:])
    pos = bound > 0
    ratio = float((head[pos] / bound[pos]).max()) if pos.any() else 0.0
    print("%s: fused %s, %d rows, value and misc max |diff| %.3g on values up to %.4g, largest ratio to the bound "
          "%.4f" % (tag, fused, len(out), head.max(), np.abs(R[:, P:]).max(), ratio))
    assert np.array_equal(got, want), tag
    assert (head <= bound).all(), (tag, ratio)


@pytest.mark.parametrize("name,precision", COMBOS, ids=["%s-%s" % c for c in COMBOS])
def test_policy_bit_equal_to_float64(model_dir, name, precision):
    c = ex.CASES[name]
    d = ex.case_data(name, model_dir)
    P, A = d["P"], c["X"] * c["Y"]
    packed = pack_u64(d["planes"])
    net = _network(d["path"], c, precision)
    fused, runs = net.fused, net.precision[0]
    if name == "b6c96-5x5-e4m3" and precision in ("corrected", "default"):
        # no operand past e4m3's 448: the calibration keeps the corrected instance, and no
        # board is re-evaluated on the split one
        assert fused and runs == "corrected", runs
    n = len(packed)
    batches = [slice(0, n)]
    if name == "b6c96-5x5-instances":
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert n > 5 * cus, "the batch does not reach the 8-board instance on %d CUs" % cus
        batches += [slice(n - 203, n), slice(n - 1, n)]
    outs = [net.forward(packed[rows]) for rows in batches]
    net.close()
    for rows, out in zip(batches, outs):
        tag = "%s %s (runs %s) rows [%d, %d)" % (name, precision, runs, rows.start, rows.stop)
        _check(tag, out, d["R"][rows], d["bound"][rows], P, A, fused)


@pytest.mark.parametrize("name,precision", [("b6c96-5x5", "fast"), ("c80m48-5x5-padded", "fast-layered")])
def test_forward_canonical_bit_equal_to_float64(model_dir, name, precision):
    """Rows declared under symmetry s come back with the policy in the canonical frame: the
    reference mapped back through the oracle-derived symmetry maps, bit for bit."""
    c = ex.CASES[name]
    d = ex.case_data(name, model_dir)
    P, A = d["P"], c["X"] * c["Y"]
    n = len(d["R"])
    sym = (np.arange(n) % 8).astype(np.int32)
    src = symmetry.canonical_source(c["X"], c["Y"], c["W"])
    assert not np.array_equal(src[sym[1]], np.arange(P))
    net = _network(d["path"], c, precision)
    fused = net.fused
    assert fused == (precision == "fast")
    out = net.forward_canonical(pack_u64(d["planes"]), sym)
    net.close()
    R = d["R"].copy()
    R[:, :P] = np.take_along_axis(R[:, :P], src[sym], axis=1)
    _check("%s %s canonical" % (name, precision), out, R, d["bound"], P, A, fused)


def _unpack(packed, X, Y):
    bits = np.unpackbits(np.ascontiguousarray(packed).view(np.uint8).reshape(len(packed), -1), axis=1,
                         bitorder="little")
    return bits[:, :15 * X * Y].reshape(len(packed), 15, Y, X).astype(np.float32)


def test_selfplay_batch_protocol_rows_are_the_reference(model_dir):
    """Self-play reaches the network through the device-side count and the row indirection.
    The oracle's search is fed the plain forward of its own batches -- each asserted bit-equal
    to the float64 reference in the policy and within the bound in the heads -- while the
    device engine plays the same games end to end: bit-identical trees and root policies say
    the protocol's rows are the plain forward's rows."""
    name = "b6c96-5x5"
    c = ex.CASES[name]
    d = ex.case_data(name, model_dir)
    X, Y, W, P = c["X"], c["Y"], c["W"], d["P"]
    G, visits, cap = 12, 16, 4 * 16 + 32
    net = _network(d["path"], c, "fast")
    fused = net.fused
    calls = []

    def device_net(packed):
        out = net.forward(packed)
        planes = _unpack(packed, X, Y)
        R, rec = ex.forward(d["net"], planes, np.full((len(planes), 1), float(W), np.float32), keep="last")
        bound, _ = ex.head_bound(d["net"], rec)
        assert np.array_equal(out[:, :P], R[:, :P].astype(np.float32)), "batch %d" % len(calls)
        assert (np.abs(out[:, P:] - R[:, P:]) <= bound).all(), "batch %d" % len(calls)
        calls.append(len(packed))
        return out

    gpu = kc.Selfplay(X, Y, W, num_games=G, max_visits=visits, seed=41, model_path=d["path"], node_cap=cap,
                      commit_interval=1, nn_cache_log2=10, nn_precision="fast")
    ora = oracle.Selfplay(X, Y, W, games=G, max_visits=visits, node_cap=cap, seed=41, nn_cache_log2=10)
    ora.set_net(device_net)
    done = 0
    for chunk in (1, 17, 40):
        gpu.step(chunk - done)
        ora.rounds(chunk - done)
        done = chunk
        gpu.sync()
        for g in range(G):
            gn, ge = gpu.game_tree(g)
            on, oe = ora.game_tree(g)
            np.testing.assert_array_equal(gn, on, err_msg="round %d game %d nodes" % (done, g))
            np.testing.assert_array_equal(ge, oe, err_msg="round %d game %d edges" % (done, g))
            if gpu.game_info(g)["phase"] == 1:
                np.testing.assert_array_equal(gpu.root_policy(g), ora.root_noised(g))
    st = gpu.stats()
    gpu.close()
    net.close()
    print("self-play on the exact b6c96 net: fused %s, %d network batches of %d..%d rows, %d evaluations" % (
        fused, len(calls), min(calls), max(calls), st["nn_evals"]))
    assert st["errors"] == 0 and st["nn_evals"] > 0 and len(calls) >= 30


def test_control_one_zeroed_tap_is_seen(model_dir):
    """The comparison can fail: with one tap of one mid-trunk 3x3 zeroed in the file, the
    fast-layered output is not the unmutated reference (it is the mutated net's)."""
    name = "c80m48-5x5-padded"
    c = ex.CASES[name]
    d = ex.case_data(name, model_dir)
    P = d["P"]
    site, mutation = "blocks.0.inner.1.conv1", ("tap", 5)
    bad = ex.mutated(d["net"], site, mutation)
    path = os.path.join(str(model_dir), "exact-%s-one-tap-zeroed.cfnn" % name)
    train.save_cfnn(bad, path)
    net = _network(path, c, "fast-layered")
    out = net.forward(pack_u64(d["planes"]))
    net.close()
    Rm, _ = ex.forward(bad, d["planes"], d["glob"])
    differ = int((out[:, :P] != d["R"][:, :P].astype(np.float32)).sum())
    print("control: %d of %d policy logits differ from the unmutated reference" % (differ, out[:, :P].size))
    assert differ > 0
    assert np.array_equal(out[:, :P], Rm[:, :P].astype(np.float32))
