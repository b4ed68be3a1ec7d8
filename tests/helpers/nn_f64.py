"""A float64 reference of the network with operand-loss probes (CPU, plain torch).

The accurate ("split") kernels carry every convolution operand as an fp16 pair hi + lo and
form each product as hi*hi + lo(w)*hi(x) + hi(w)*lo(x).  If the second product went missing
somewhere, the result there would be what fp16-rounded weights give; if the third went
missing, what fp16-rounded activations give.  This module computes exactly those outputs
with ``train.CoffeeNet`` in float64: it wraps the matmul sites of ``katacoffee_amd.train``
(the ``F.conv2d`` calls and the ``"nchw,oc->nohw"`` einsums), numbers them in call order and
rounds a chosen part of one site's chosen operand to fp16 (round to nearest even).

  reference(path, planes, glob)      R: [n][4A + 4] float64 (policy, value, misc)
  probing(probes)                    the context manager; ``.sites`` lists the sites met
  sites(net, X, Y)                   [(index, parameter name, kind, input width)]
  signatures(net, planes, glob, probes)   max |R_probe - R| per probe, and e32
  plan(net, X, Y, ...)               the probe list of a test case

A probe is ``(site, operand, part)``: operand ``"w"`` or ``"x"``; part ``("all",)``,
``("tap", t)`` (tap t = 3 ky + kx of a 3x3) or ``("slice", j)`` (input channels
[32 j, 32 j + 32)).  For the activation side of a partial probe the site computes
f(x, w (1 - m)) + f(q16(x), w m), m the part's mask in w.

The cases the CPU and GPU tests share (nets, geometries, batches, probe plans) are in CASES.
"""
import contextlib
import copy
import os

import numpy as np
import torch
import torch.nn.functional as F

from katacoffee_amd import train
from oracle import oracle

EINSUM = "nchw,oc->nohw"
MAX_THREADS = 8


def q16(t):
    """fp16 rounding (RNE) of a float64 / float32 tensor, in its own dtype."""
    return t.to(torch.float16).to(t.dtype)


@contextlib.contextmanager
def _threads():
    old = torch.get_num_threads()
    torch.set_num_threads(max(1, min(old, MAX_THREADS)))
    try:
        yield
    finally:
        torch.set_num_threads(old)


class _Shim:
    """Stands in for a module bound in train's namespace: one attribute replaced."""

    def __init__(self, real, name, fn):
        self._real = real
        setattr(self, name, fn)

    def __getattr__(self, k):
        return getattr(self._real, k)


def _mask(w, part):
    m = torch.zeros_like(w)
    if part[0] == "all":
        m[...] = 1.0
    elif part[0] == "tap":
        assert w.dim() == 4 and 0 <= part[1] < 9
        m[:, :, part[1] // 3, part[1] % 3] = 1.0
    elif part[0] == "slice":
        assert 32 * part[1] < w.shape[1]
        m[:, 32 * part[1]:32 * part[1] + 32] = 1.0
    else:
        raise ValueError("unknown probe part %r" % (part,))
    return m


class _Probing:
    def __init__(self, probes):
        self.by_site = {}
        for site, operand, part in probes:
            assert operand in ("w", "x")
            self.by_site.setdefault(site, []).append((operand, tuple(part)))
        self.sites = []  # (index, kind, weight tensor) in call order

    def _site(self, kind, f, x, w):
        i = len(self.sites)
        self.sites.append((i, kind, w))
        todo = self.by_site.get(i)
        if not todo:
            return f(x, w)
        wd = w.detach()
        for operand, part in todo:
            if operand == "w":
                m = _mask(wd, part)
                wd = wd * (1.0 - m) + q16(wd) * m
        xs = [part for operand, part in todo if operand == "x"]
        if not xs:
            return f(x, wd)
        m = torch.zeros_like(wd)
        for part in xs:
            m = torch.maximum(m, _mask(wd, part))
        if bool((m == 1.0).all()):
            return f(q16(x), wd)
        return f(x, wd * (1.0 - m)) + f(q16(x), wd * m)

    def conv2d(self, x, w, *args, **kw):
        return self._site("conv3", lambda a, b: F.conv2d(a, b, *args, **kw), x, w)

    def einsum(self, eq, *ops):
        if eq != EINSUM:
            return torch.einsum(eq, *ops)
        return self._site("conv1", lambda a, b: torch.einsum(eq, a, b), ops[0], ops[1])


@contextlib.contextmanager
def probing(probes=()):
    """Wraps train's matmul sites for the duration; yields the recorder (``.sites``)."""
    p = _Probing(probes)
    real_F, real_torch = train.F, train.torch
    train.F = _Shim(real_F, "conv2d", p.conv2d)
    train.torch = _Shim(real_torch, "einsum", p.einsum)
    try:
        yield p
    finally:
        train.F, train.torch = real_F, real_torch


def _forward(net, planes, glob, probes=()):
    dt = next(net.parameters()).dtype
    b = torch.as_tensor(np.ascontiguousarray(planes)).to(dt)
    g = torch.as_tensor(np.ascontiguousarray(glob)).to(dt).reshape(b.shape[0], -1)
    with torch.no_grad(), _threads(), probing(probes) as p:
        pol, val, misc = net(b, g)
    return torch.cat([pol, val, misc], dim=1).to(torch.float64).numpy(), p


def load(path):
    return train.load_cfnn(path).double()


def reference(path, planes, glob):
    """planes [n][15][Y][X] {0,1}, glob [n][1] -> [n][4A + 4] float64."""
    return _forward(load(path), planes, glob)[0]


def sites(net, X, Y):
    """[(index, name, kind, input width)] of the net's matmul sites, in call order."""
    names = {id(p): n for n, p in net.named_parameters()}
    planes = np.zeros((1, net.cfg["cin"], Y, X), np.float32)
    _, p = _forward(net, planes, np.zeros((1, net.cfg["gin"]), np.float32))
    return [(i, names[id(w)], kind, int(w.shape[1])) for i, kind, w in p.sites]


# Probes the device cannot lose, by name of the site's weight: no rounded operand exists there.
#  convInit x: the stem's inputs are the 0/1 planes, exact in fp16 (lo(x) == 0);
#  pConv2:     the policy's second 1x1 is evaluated in f32 outside the MFMAs (kHeadsL,
#              and the fused kernel's head phase).
def excluded(name, operand):
    if name == "convInit" and operand == "x":
        return "stem inputs are 0/1, exact in fp16"
    if name == "pConv2":
        return "evaluated in f32 outside the MFMAs"
    return None


def plan(net, X, Y, whole=True, taps=None, slices=None):
    """The probe list [(probe, label)]: whole sites (every retained one), and per tap /
    per slice for the sites whose name `taps` / `slices` accept (callables on the name)."""
    out = []
    for i, name, kind, cin in sites(net, X, Y):
        for operand in ("w", "x"):
            if excluded(name, operand):
                continue
            if whole:
                out.append(((i, operand, ("all",)), "%s.%s" % (name, operand)))
            if kind == "conv3" and taps and taps(name):
                for t in range(9):
                    out.append(((i, operand, ("tap", t)), "%s.%s.tap%d" % (name, operand, t)))
            if slices and slices(name):
                for j in range((cin + 31) // 32):
                    out.append(((i, operand, ("slice", j)), "%s.%s.slice%d" % (name, operand, j)))
    return out


def both_sides(net, X, Y):
    """Every retained site rounded on both sides: what the fp16 kernels compute (and the
    oracle's fp16-emulation mode 1, which rounds every convolution's weights and inputs)."""
    return [(i, op, ("all",)) for i, name, _, _ in sites(net, X, Y) if name != "pConv2" for op in ("w", "x")]


def signatures(net, planes, glob, probes):
    """R, [max |R_probe - R|] per probe, e32 = max |float32 forward - R|."""
    R, _ = _forward(net, planes, glob)
    sig = np.array([float(np.abs(_forward(net, planes, glob, [p])[0] - R).max()) for p in probes])
    r32, _ = _forward(copy.deepcopy(net).float(), planes, glob)
    return R, sig, float(np.abs(r32 - R).max())


# -- nets and inputs -----------------------------------------------------------------
def make_net(cfg, seed, sigma=0.1):
    """He-initialised CoffeeNet with every 1-D parameter (norm scales and biases, head
    biases) perturbed by N(0, sigma), so no bias or norm term is trivial."""
    net = train.CoffeeNet(cfg)
    net.reset_parameters(seed)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=g) * sigma)
    return net


def boards(n, X, Y, W, seed):
    """n positions: random stones with up to 5 history moves and a random symmetry, the
    last two the empty board and a board with every cell occupied.  -> planes
    [n][15][Y][X] f32, glob [n][1] f32."""
    rng = np.random.default_rng(seed)
    A = X * Y
    colors = np.zeros((n, A), np.uint8)
    hc = np.full((n, 5), -1, np.int8)
    hd = np.full((n, 5), 4, np.int8)
    for i in range(n - 2):
        k = int(rng.integers(1, A // 2))
        idx = rng.choice(A, size=k, replace=False)
        colors[i, idx] = rng.integers(1, 3, size=k)
        h = min(k, int(rng.integers(0, 6)))
        hc[i, :h] = idx[:h]
        hd[i, :h] = rng.integers(0, 4, size=h)
    colors[n - 1] = 1 + (np.arange(A) % 2)
    pla = rng.integers(1, 3, size=n).astype(np.uint8)
    sym = rng.integers(0, 8, size=n).astype(np.int32)
    binp, glob = oracle.encode_batch(X, Y, W, colors, hc, hd, pla, sym)
    return binp.reshape(n, -1, Y, X).astype(np.float32), glob.reshape(n, 1).astype(np.float32)


def pack_u64(planes):
    """[n][15][Y][X] {0,1} -> [n][ceil(15A/64)] u64, bit i of the flat index in word i>>6."""
    n = planes.shape[0]
    flat = planes.reshape(n, -1).astype(np.uint8)
    words = (flat.shape[1] + 63) // 64
    bits = np.zeros((n, words * 64), np.uint8)
    bits[:, :flat.shape[1]] = flat
    return np.packbits(bits, axis=1, bitorder="little").view("<u8").reshape(n, words)


# -- the shared cases ----------------------------------------------------------------
_ALL = lambda name: True  # noqa: E731
_B6_PARTS = lambda name: name.startswith("blocks.0.") or name.startswith("blocks.2.")  # noqa: E731
_ONE_BY_ONE = lambda name: name.endswith("convP") or name.endswith("convQ")  # noqa: E731

_HEADS_SMALL = dict(p1=32, g1=32, v1=32, v2=64)
CASES = {
    # name: net (architecture name or config), geometry, boards (ragged against the
    # instance's boards per workgroup), seed, probe plan, precisions under test, control.
    # The seed (of the net and of the positions) is chosen on the CPU alone, so that the
    # smallest signature is well above 8 x the float32 forward's own error
    # (test_nn_f64_reference.py asserts it); no device result enters the choice.
    "b6c96-5x5": dict(cfg="b6c96", X=5, Y=5, W=4, n=7, seed=1, taps=_B6_PARTS, slices=_B6_PARTS,
                      accurate=["accurate"], fast="fast"),
    "b6c96-5x5-nb2": dict(cfg="b6c96", X=5, Y=5, W=4, n=3, seed=1, taps=_B6_PARTS, slices=_B6_PARTS,
                          accurate=["accurate-nb2"], fast="fast"),
    "b6c96-7x7": dict(cfg="b6c96", X=7, Y=7, W=5, n=7, seed=2, accurate=["accurate"], fast="fast-layered"),
    "c64-5x5-tn2": dict(cfg=dict(C=64, Cg=16, kinds=[0], **_HEADS_SMALL), X=5, Y=5, W=4, n=13, seed=3, taps=_ALL,
                        slices=_ALL, accurate=["accurate"], fast="fast-layered"),
    "c96g32-7x7-tn3": dict(cfg=dict(C=96, Cg=32, kinds=[1], **_HEADS_SMALL), X=7, Y=7, W=5, n=7, seed=4, taps=_ALL,
                           slices=_ALL, accurate=["accurate"], fast="fast-layered"),
    "c128-9x9-tn4": dict(cfg=dict(C=128, Cg=32, kinds=[0], **_HEADS_SMALL), X=9, Y=9, W=5, n=4, seed=35, taps=_ALL,
                         slices=_ALL, accurate=["accurate"], fast="fast-layered"),
    "c384m192-9x9": dict(cfg=dict(C=384, mid=192, Cg=64, p1=48, g1=48, v1=96, v2=128, kinds=[3, 2]), X=9, Y=9, W=5,
                         n=4, seed=16, slices=_ONE_BY_ONE, accurate=["accurate"], fast="fast-layered"),
    "c80m48-5x5-padded": dict(cfg=dict(C=80, mid=48, Cg=24, p1=24, g1=20, v1=40, v2=72, kinds=[3]), X=5, Y=5, W=4,
                              n=13, seed=7, taps=_ALL, slices=_ALL, accurate=["accurate"], fast="fast-layered"),
    "b10c128-7x7-default": dict(cfg="b10c128", X=7, Y=7, W=5, n=7, seed=8, accurate=["default"],
                                fast="fast-layered"),
    # the layered constructor's limits together
    "limits-5x5": dict(cfg=dict(C=160, Cg=128, p1=64, g1=64, v1=128, v2=256, kinds=[1, 0]), X=5, Y=5, W=4, n=13,
                       seed=9, accurate=["accurate"], fast="fast-layered"),
    # the layered kernels' granularity: trunk and bottleneck widths any multiple of 4, every
    # other width free (odd head and gpool widths)
    "c68m36-5x5-odd": dict(cfg=dict(C=68, mid=36, Cg=11, p1=21, g1=13, v1=37, v2=41, kinds=[3, 1]), X=5, Y=5, W=4,
                           n=13, seed=10, accurate=["accurate"], fast="fast-layered"),
}
# the named architectures also run the engine's own random-init net (kc.write_random_model)
RANDOM_INIT = {"b6c96-5x5": 0xC0FFEE, "b6c96-5x5-nb2": 0xC0FFEE, "b6c96-7x7": 0xC0FFEE,
               "b10c128-7x7-default": 0xC0FFEE}

_cache = {}


def case_data(name, model_dir, random_init=False):
    """Writes the case's net to model_dir and computes, once per process: path, planes,
    glob, R, probe labels, signatures, e32."""
    key = (name, random_init)
    if key in _cache and os.path.exists(_cache[key]["path"]):
        return _cache[key]
    c = CASES[name]
    path = os.path.join(str(model_dir), "%s%s.cfnn" % (name, "-rand" if random_init else ""))
    if random_init:
        import katacoffee_amd as kc
        kc.write_random_model(c["cfg"], RANDOM_INIT[name], path)
    else:
        train.save_cfnn(make_net(c["cfg"], c["seed"]), path)
    net = load(path)
    planes, glob = boards(c["n"], c["X"], c["Y"], c["W"], seed=c["seed"])
    pl = plan(net, c["X"], c["Y"], whole=True, taps=c.get("taps"), slices=c.get("slices"))
    R, sig, e32 = signatures(net, planes, glob, [p for p, _ in pl])
    d = dict(path=path, planes=planes, glob=glob, R=R, labels=[l for _, l in pl], probes=[p for p, _ in pl], sig=sig,
             e32=e32, net=net)
    _cache[key] = d
    return d
