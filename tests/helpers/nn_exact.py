"""Integer-valued networks with exactly one possible policy output (CPU, plain torch).

Activations are ReLU, norms per-channel affine, inputs 0/1 planes.  A net with small integer
weights, unit norm scales and integer biases keeps every activation an integer; while every
matmul operand is an integer below 2048 in magnitude it equals its fp16 rounding (lo = 0 in
the split and the corrected schemes), and while every output's sum of |w x| stays below
2^24 every f32 summation order gives the same sum.  Such a net has ONE policy output: the
fused and the layered kernels, every precision and every instance must produce it bit for
bit, equal to ``train.CoffeeNet`` in float64.  No tolerance, no accumulation order.

  make_exact_net(cfg, seed, X, Y, k, wmax, ...)   the net (float32 CoffeeNet; save with train.save_cfnn)
  boards(n, X, Y, W, seed)                   nn_f64.boards plus two border-only boards
  forward(net, planes, glob, ...)            float64 forward: R, per-site records
  mutations(net, X, Y, ...)                  [(mutation, label)]: site / tap / slice / tile / transpose
  mutated(net, site_name, mutation)          a copy of the net with the mutation in its weights
  head_bound(net, rec)                       the value head's a-priori f32 summation bound
  CASES, case_data(name, model_dir)          the cases the CPU and the GPU tests share

Construction (per matmul site of nn_f64.sites): weights uniform in {-wmax..wmax} \\ {0} at
density min(1, k / fan_in), plus one +-1 for every input channel no output would read (so
that whatever the layer before computes can reach the logits), and at least MIN_PER_TAP
weights per tap of a narrow 3x3; every norm scale 1; every 1-D bias an integer in [-1, 1]
([0, 1] for b18c384nbt); the other 2-D linears sparse +-1.  In the trunk and policy gpool linears (linG, pLinG) the mean
and the mean-times-constant columns are zero: mean = S / A is not exact for A = 25, 49, 81
and those columns feed fp16 operands; the max columns stay.  The value head's gpool is means
only, so value and misc are not exact: head_bound() gives their bound.

What the conditions are (tests/test_nn_exact_reference.py asserts them on the CPU, with no
kernel) is in ``conditions``; k, wmax and the seed of a case are chosen there, never from a
device result.
"""
import copy
import importlib.util
import os

import numpy as np
import torch
import torch.nn.functional as F

from katacoffee_amd import train
from oracle import oracle

_spec = importlib.util.spec_from_file_location("nn_f64", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                      "nn_f64.py"))
f64 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(f64)

SCALES = ("bnPs", "bnQs", "bn1s", "bngs", "bn2s", "tips")
GPOOL_LINEARS = ("linG", "pLinG")
FORWARDS = [0]  # float64 forwards run so far (the CPU test prints it)


# -- the net -----------------------------------------------------------------------------
MIN_PER_TAP = 8  # a narrow 3x3 (a gpool branch, a bottleneck's inner conv1) keeps this many weights per tap


def _sparse(shape, fan_in, k, wmax, g):
    if len(shape) == 4:
        k = max(k, 9.0 * MIN_PER_TAP / shape[0])
    keep = torch.rand(shape, generator=g) < min(1.0, k / fan_in)
    mag = torch.randint(1, wmax + 1, shape, generator=g).float()
    sign = torch.randint(0, 2, shape, generator=g).float() * 2.0 - 1.0
    w = keep.float() * mag * sign
    # every input channel is read by some output (at a random tap): what the layer before
    # computes in that channel can reach the logits
    flat = w.view(shape[0], shape[1], -1)
    for c in torch.nonzero(flat.abs().sum(dim=(0, 2)) == 0).flatten().tolist():
        o = int(torch.randint(0, shape[0], (1,), generator=g))
        t = int(torch.randint(0, flat.shape[2], (1,), generator=g))
        flat[o, c, t] = float(torch.randint(0, 2, (1,), generator=g)) * 2.0 - 1.0
    return w


def make_exact_net(cfg, seed, X, Y, k=3, wmax=1, k_head=None, bias_min=-1):
    """A CoffeeNet whose parameters are overwritten from a seeded generator as the module
    docstring says.  k: expected nonzero weights per output of a matmul site; wmax: their
    largest magnitude; k_head: k of the heads' sites (pConv1, pConvG, pConv2, vConv1) and of
    the heads' other linears, for the deep nets whose trunk allows little; bias_min: the
    biases are integers in [bias_min, 1] (0 keeps a deep sparse net's activations alive: with
    -1 most entries sit below the ReLU and a small change dies within a few layers)."""
    net = train.CoffeeNet(cfg)
    site_names = {name for _, name, _, _ in f64.sites(net, X, Y)}
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            last = name.split(".")[-1]
            if p.dim() == 1:
                if last in SCALES:
                    p.fill_(1.0)
                else:
                    p.copy_(torch.randint(bias_min, 2, p.shape, generator=g).float())
            elif name in site_names:
                head = k_head is not None and "." not in name and name != "convInit"
                p.copy_(_sparse(p.shape, p[0].numel(), k_head if head else k, wmax, g))
            elif last in GPOOL_LINEARS:
                third = p.shape[1] // 3  # columns: mean, mean x constant, max
                p.zero_()
                p[:, 2 * third:].copy_(_sparse((p.shape[0], third), third, k, 1, g))
            else:
                p.copy_(_sparse(p.shape, p[0].numel(), k_head or k, 1, g))
    return net


def boards(n, X, Y, W, seed):
    """nn_f64.boards(n) (random positions, the empty and the full board) and two boards with
    stones on the border cells only, so that the padding matters at every edge: one with
    the colours alternating along the border, one of a single colour with history moves in
    the corners.  -> planes [n + 2][15][Y][X] f32, glob [n + 2][1] f32."""
    planes, glob = f64.boards(n, X, Y, W, seed)
    A = X * Y
    yy, xx = np.divmod(np.arange(A), X)
    border = np.flatnonzero((yy == 0) | (yy == Y - 1) | (xx == 0) | (xx == X - 1))
    colors = np.zeros((2, A), np.uint8)
    colors[0, border] = 1 + (np.arange(len(border)) % 2)
    colors[1, border] = 2
    hc = np.full((2, 5), -1, np.int8)
    hd = np.full((2, 5), 4, np.int8)
    hc[1, :4] = [0, X - 1, A - X, A - 1]
    hd[1, :4] = [0, 1, 2, 3]
    binp, gl = oracle.encode_batch(X, Y, W, colors, hc, hd, np.array([1, 2], np.uint8), np.array([0, 5], np.int32))
    return (np.concatenate([planes, binp.reshape(2, -1, Y, X).astype(np.float32)]),
            np.concatenate([glob, gl.reshape(2, 1).astype(np.float32)]))


# -- float64 forward with a recorder, mutations and replay, on nn_f64's shims --------------
def _mutate(w, mutation):
    """The mutated copy of a site's weights."""
    kind = mutation[0]
    if kind == "transpose":
        assert w.dim() == 4
        return w.transpose(2, 3).contiguous()
    w = w.clone()
    if kind == "site":
        w.zero_()
    elif kind == "tap":
        assert w.dim() == 4 and 0 <= mutation[1] < 9
        w[:, :, mutation[1] // 3, mutation[1] % 3] = 0.0
    elif kind == "slice":
        assert 32 * mutation[1] < w.shape[1]
        w[:, 32 * mutation[1]:32 * mutation[1] + 32] = 0.0
    elif kind == "tile":
        assert 16 * mutation[1] < w.shape[0]
        w[16 * mutation[1]:16 * mutation[1] + 16] = 0.0
    else:
        raise ValueError("unknown mutation %r" % (mutation,))
    return w


class _Recorder(f64._Probing):
    """record: per site max |x|, fp16-exactness of x and w, max over outputs of f(|x|, |w|),
    the nonzero share of x and the emptiest 32-channel slice of x.  mutate: (site, mutation).
    replay: {site: output} returned in place of the sites before the mutated one; keep: the
    outputs are stored (for a later replay)."""

    def __init__(self, record=False, mutate=None, replay=None, keep=False):
        super().__init__(())
        self.record, self.mutate, self.replay, self.keep = record, mutate, replay, keep
        self.outputs = {} if keep else None
        self.records = []

    def _site(self, kind, f, x, w):
        i = len(self.sites)
        self.sites.append((i, kind, w))
        if self.replay is not None and self.mutate is not None and i < self.mutate[0]:
            return self.replay[i]
        wd = w.detach()
        if self.mutate is not None and i == self.mutate[0]:
            wd = _mutate(wd, self.mutate[1])
        y = f(x, wd)
        if self.outputs is not None:
            if self.keep == "last":
                self.outputs.clear()
            self.outputs[i] = y
        if self.record:
            nz = (x != 0).transpose(0, 1).flatten(1).any(dim=1)  # [c]: the channel is lit somewhere
            per_slice = [int(nz[j:j + 32].sum()) for j in range(0, x.shape[1], 32)]
            self.records.append(dict(
                site=i, kind=kind, max_x=float(x.abs().max()), max_w=float(wd.abs().max()),
                x_fp16=bool((f64.q16(x) == x).all()), w_fp16=bool((f64.q16(wd) == wd).all()),
                x_int=bool((x == x.round()).all()), sum_abs=float(f(x.abs(), wd.abs()).max()),
                nonzero=float((x != 0).double().mean()), min_slice_channels=min(per_slice)))
        return y


def forward(net, planes, glob, record=False, mutate=None, replay=None, keep=False):
    """-> R [n][4A + 4] float64 and the recorder (.records, .outputs)."""
    assert next(net.parameters()).dtype == torch.float64
    rec = _Recorder(record, mutate, replay, keep)
    b = torch.as_tensor(np.ascontiguousarray(planes)).double()
    g = torch.as_tensor(np.ascontiguousarray(glob)).double().reshape(b.shape[0], -1)
    real_F, real_torch = train.F, train.torch
    train.F = f64._Shim(real_F, "conv2d", rec.conv2d)
    train.torch = f64._Shim(real_torch, "einsum", rec.einsum)
    try:
        with torch.no_grad(), f64._threads():
            pol, val, misc = net(b, g)
    finally:
        train.F, train.torch = real_F, real_torch
    FORWARDS[0] += 1
    return torch.cat([pol, val, misc], dim=1).numpy(), rec


def mutated(net, site_name, mutation):
    """A copy of the net with the mutation applied to the named site's weights."""
    m = copy.deepcopy(net)
    p = dict(m.named_parameters())[site_name]
    with torch.no_grad():
        p.copy_(_mutate(p.detach(), mutation))
    return m


def mutations(net, X, Y, thin=False):
    """[((site, mutation), label)]: whole site, every tap and the tap transpose at every site;
    every 32-input-channel slice and every 16-output-channel tile at every site -- with
    `thin`, slices and tiles only at the first, a middle and the last site of each kind."""
    ss = f64.sites(net, X, Y)
    parts_at = set(i for i, _, _, _ in ss)
    if thin:
        parts_at = set()
        for kind in ("conv3", "conv1"):
            idx = [i for i, _, k, _ in ss if k == kind]
            parts_at |= {idx[0], idx[len(idx) // 2], idx[-1]}
    weights = {n: p for n, p in net.named_parameters()}
    out = []
    for i, name, kind, cin in ss:
        out.append(((i, ("site",)), "%s.site" % name))
        if kind == "conv3":
            out += [((i, ("tap", t)), "%s.tap%d" % (name, t)) for t in range(9)]
            out.append(((i, ("transpose",)), "%s.transpose" % name))
        if i in parts_at:
            out += [((i, ("slice", j)), "%s.slice%d" % (name, j)) for j in range((cin + 31) // 32)]
            cout = weights[name].shape[0]
            out += [((i, ("tile", j)), "%s.tile%d" % (name, j)) for j in range((cout + 15) // 16)]
    return out


# -- the value head's bound ---------------------------------------------------------------
def head_bound(net, rec):
    """n 2^-24 S per value and misc output [rows][4]: S the float64 forward of the head's f32
    linears on absolute values (|vLin3| or |vLinM| on |vLin2| |gpool| + |vB2|, plus the last
    bias), n the longest dot product in the head (3 v1 or v2) plus 4: the a-priori bound of
    f32 summation, whatever its order.  The head's input v (vConv1's ReLU output) is exact.
    rec: the recorder of a forward that kept vConv1's output (keep="last")."""
    v1, v2 = net.cfg["v1"], net.cfg["v2"]
    with torch.no_grad():
        return _head_bound(net, rec, v1, v2)


def _head_bound(net, rec, v1, v2):
    v = F.relu(rec.outputs[len(rec.sites) - 1] + net.vBias1[:, None, None])  # vConv1 is the last site
    pool = train._gpool(v, value_head=True).abs()
    h = pool @ net.vLin2.abs().t() + net.vB2.abs()
    S = torch.cat([h @ net.vLin3.abs().t() + net.vB3.abs(), h @ net.vLinM.abs().t() + net.vBM.abs()], dim=1)
    n = max(3 * v1, v2) + 4
    return (n * 2.0 ** -24 * S).detach().numpy(), n


# -- the conditions -----------------------------------------------------------------------
def conditions(records, R, P, max_x=2048):
    """The list of the input conditions a case fails (empty: the case is usable).  max_x: the
    bound on |operand| (2048: exact in fp16; a case may ask for less)."""
    bad = []
    for r in records:
        tag = "site %d" % r["site"]
        if not (r["x_fp16"] and r["w_fp16"]):
            bad.append("%s: an operand is not its fp16 rounding" % tag)
        if not r["x_int"]:
            bad.append("%s: a non-integer activation" % tag)
        if not r["max_x"] < max_x:
            bad.append("%s: max |x| %g" % (tag, r["max_x"]))
        if not r["sum_abs"] < 2 ** 24:
            bad.append("%s: max sum |w x| %g" % (tag, r["sum_abs"]))
        if not r["min_slice_channels"] >= 1:
            bad.append("%s: a 32-channel input slice is all zero" % tag)
        if not r["nonzero"] >= 0.10:
            bad.append("%s: only %.1f %% of the inputs are nonzero" % (tag, 100 * r["nonzero"]))
    pol = R[:, :P]
    if not (pol == np.round(pol)).all():
        bad.append("a policy logit is not an integer")
    if not np.abs(pol).max() < 2 ** 24:
        bad.append("a policy logit is not exact in f32")
    rows = pol[:DISTINCT_ROWS]
    if not len(np.unique(rows)) >= rows.size / 4:
        bad.append("only %d distinct values among %d policy logits" % (len(np.unique(rows)), rows.size))
    return bad


# The distinct-values condition looks at a case's first rows: integer logits of magnitude
# below 2^11 cannot take 1e5 distinct values on the 1319-row batch.
DISTINCT_ROWS = 16

# -- the shared cases ----------------------------------------------------------------------
# The batch that reaches the fused 8-board instance needs more than 5 boards per CU: 256 CUs.
N_BIG = 5 * 256 + 37


def _case(base, **over):
    c = f64.CASES[base]
    return dict(dict(cfg=c["cfg"], X=c["X"], Y=c["Y"], W=c["W"], n=c["n"]), **over)


CASES = {
    # name: net, geometry, nn_f64.boards' count (two border boards are added), then what the
    # CPU conditions chose: k, wmax, seed; thin: slices and tiles at three sites per kind
    "b6c96-5x5": _case("b6c96-5x5", k=2.5, wmax=1, seed=3),
    # every operand within e4m3's 448: the corrected instance flags no board as hot, so its own
    # output is compared and not the split re-evaluation's
    "b6c96-5x5-e4m3": _case("b6c96-5x5", k=2, wmax=1, seed=6, max_x=449),
    "b6c96-5x5-nb2": _case("b6c96-5x5-nb2", k=2.5, wmax=1, seed=3),
    # the same net on the batches test_network_row_independence uses: all rows (the fused
    # 8-board instance), the last 203 (the 5-board one) and the last row alone
    "b6c96-5x5-instances": _case("b6c96-5x5", n=N_BIG, k=2.5, wmax=1, seed=3, mutate=False),
    "b6c96-7x7": _case("b6c96-7x7", k=2.5, wmax=1, seed=5),
    "c64-5x5-tn2": _case("c64-5x5-tn2", k=8, wmax=2, seed=3),
    "c96g32-7x7-tn3": _case("c96g32-7x7-tn3", k=6, wmax=2, seed=4),
    "c128-9x9-tn4": _case("c128-9x9-tn4", k=8, wmax=2, seed=5),
    "c384m192-9x9": _case("c384m192-9x9", k=2.5, wmax=1, seed=6),
    "c80m48-5x5-padded": _case("c80m48-5x5-padded", k=6, wmax=1, seed=7),
    "limits-5x5": _case("limits-5x5", k=6, wmax=1, seed=9),
    "c68m36-5x5-odd": _case("c68m36-5x5-odd", k=3, wmax=1, seed=14),
    "b10c128-7x7-default": _case("b10c128-7x7-default", k=1.75, wmax=1, seed=10),
    "b2c32nbt-5x5": dict(cfg="b2c32nbt", X=5, Y=5, W=4, n=7, k=2.5, wmax=1, seed=13),
    "b18c384nbt-9x9": dict(cfg="b18c384nbt", X=9, Y=9, W=5, n=3, k=0.4, k_head=3, wmax=1, seed=13, bias_min=0,
                           thin=True),
}

_cache = {}


def case_net(name):
    c = CASES[name]
    return make_exact_net(c["cfg"], c["seed"], c["X"], c["Y"], k=c["k"], wmax=c["wmax"], k_head=c.get("k_head"),
                          bias_min=c.get("bias_min", -1))


def case_data(name, model_dir, record=False):
    """Writes the case's net to model_dir and computes, once per process: path, net (float64,
    read back from the file), planes, glob, R, the head bound [rows][4] and its n, and (with
    `record`) the per-site records."""
    key = (name, record)
    if key in _cache and os.path.exists(_cache[key]["path"]):
        return _cache[key]
    c = CASES[name]
    path = os.path.join(str(model_dir), "exact-%s.cfnn" % name)
    train.save_cfnn(case_net(name), path)
    net = f64.load(path)
    planes, glob = boards(c["n"], c["X"], c["Y"], c["W"], seed=c["seed"])
    R, rec = forward(net, planes, glob, record=record, keep="last")
    bound, n = head_bound(net, rec)
    d = dict(path=path, net=net, planes=planes, glob=glob, R=R, records=rec.records, P=4 * c["X"] * c["Y"],
             bound=bound, bound_n=n)
    _cache[key] = d
    return d
