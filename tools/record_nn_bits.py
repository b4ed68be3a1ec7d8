"""Records the fused network's output bits for tests/test_gpu_nn_bits.py.

Run once on the GPU from a build whose logits are the yardstick (the parent of a kernel
change): python tools/record_nn_bits.py  ->  tests/golden/nn_fused_bits.npz

Only kc.Network.forward and kc.Selfplay are used, so any build of the library can record.
The cases (shared with the test, which imports this file):
  * b6c96 @ 5x5, two random-init models, seeded random packed planes (6 words per board),
    precisions fast / accurate / corrected at n = 1, 5, 6, 13 boards (5 boards per
    workgroup: a partial workgroup, a full one, a second one holding one board, three with
    a partial last one): the full outputs;
  * fast at n = 5 x CUs + 1, the smallest batch that selects the 8-board instance: a
    SHA-256 of the output bytes (and the CU count it was recorded at);
  * the device-side count / row-index path: a 12-game self-play of 96 rounds on the fast
    network; SHA-256 of every drained row array, of the games' states and root policies,
    and (seven rounds later, mid-search) of every game's search tree.
"""
import hashlib
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "nn_fused_bits.npz")

MODEL_SEEDS = (0xB175, 0xC0FFEE)
PRECISIONS = ("fast", "accurate", "corrected")
SIZES = (1, 5, 6, 13)
WORDS = 6  # ceil(15 planes x 25 cells / 64)
SELFPLAY_ROUNDS = 96
ROW_KEYS = ("binaryInputNCHWPacked", "globalInputNC", "policyTargetsNCMove", "globalTargetsNC",
            "valueTargetsNCHW", "meta")


def packed_planes(n, seed):
    """[n][6] u64 of seeded random plane bits (about a quarter set; bits past 375 clear)."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 63, size=(n, WORDS), dtype=np.uint64) & \
        rng.integers(0, 1 << 63, size=(n, WORDS), dtype=np.uint64)
    w[:, WORDS - 1] &= np.uint64((1 << (15 * 25 - 64 * (WORDS - 1))) - 1)
    return w


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def write_models(kc, d):
    paths = []
    for s in MODEL_SEEDS:
        p = os.path.join(d, "b6c96_%x.cfnn" % s)
        kc.write_random_model("b6c96", s, p)
        paths.append(p)
    return paths


def small_outputs(kc, path, mi):
    """{key: [n][104] f32} for every precision and size on model index mi."""
    out = {}
    for prec in PRECISIONS:
        net = kc.Network(path, 5, 5, 4, precision=prec)
        for n in SIZES:
            out["m%d_%s_n%d" % (mi, prec, n)] = net.forward(packed_planes(n, 1000 * mi + n))
        net.close()
    return out


def big_hash(kc, path, mi, cus):
    """SHA-256 of the fast outputs at 5 x CUs + 1 boards (the 8-board instance)."""
    n = 5 * cus + 1
    net = kc.Network(path, 5, 5, 4, precision="fast")
    o = net.forward(packed_planes(n, 77 + mi))
    net.close()
    assert o.shape == (n, 104)
    return sha(o)


def selfplay_hashes(kc, path, mi):
    """[(name, sha)] of the drained rows and the game trees after the self-play window."""
    sp = kc.Selfplay(5, 5, 4, num_games=12, max_visits=16, nn_precision="fast", seed=31 + mi, model_path=path)
    sp.step(SELFPLAY_ROUNDS)
    sp.sync()
    rows = sp.drain_rows()
    res = [("rows_" + k, sha(rows[k])) for k in ROW_KEYS]
    res.append(("nrows", str(len(rows["meta"]))))
    # 96 rounds of 16 visits are six moves and no finished game: the rows above are empty
    # and the trees were just reset, so the games' states are hashed too, and the trees
    # after seven more rounds (mid-search)
    h = hashlib.sha256()
    for g in range(12):
        h.update(repr(sorted(sp.game_info(g).items())).encode())
        h.update(sp.root_policy(g).tobytes())
    res.append(("games", h.hexdigest()))
    sp.step(7)
    sp.sync()
    h = hashlib.sha256()
    nn = 0
    for g in range(12):
        nodes, edges = sp.game_tree(g, 1024)
        nn += len(nodes)
        h.update(np.ascontiguousarray(nodes).tobytes())
        h.update(np.ascontiguousarray(edges).tobytes())
    assert nn > 12, "the search trees are empty"
    res.append(("trees", h.hexdigest()))
    sp.close()
    return res


def main():
    sys.path.insert(0, REPO)
    import katacoffee_amd as kc

    gold = {}
    cus = cu_count()
    gold["cus"] = np.int64(cus)
    with tempfile.TemporaryDirectory() as d:
        for mi, path in enumerate(write_models(kc, d)):
            gold.update(small_outputs(kc, path, mi))
            gold["m%d_fast_big_sha" % mi] = np.array(big_hash(kc, path, mi, cus))
            for name, hx in selfplay_hashes(kc, path, mi):
                gold["m%d_sp_%s" % (mi, name)] = np.array(hx)
                print("model %d selfplay %s %s" % (mi, name, hx))
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **gold)
    print("wrote %s (%d bytes, %d CUs)" % (GOLDEN, os.path.getsize(GOLDEN), cus))


if __name__ == "__main__":
    main()
