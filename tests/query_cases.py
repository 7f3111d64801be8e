"""Seeded inputs shared by tests/golden/make_query_golden.py (which runs the reference's own code on them),
tests/test_query_host.py (which checks their margin conditions on the CPU) and tests/test_38_query_gpu.py (which runs the
kernels on them).  Nothing here reads a file."""
import numpy as np

GOLD_K, GOLD_ROOTS, GOLD_D, GOLD_Q, GOLD_N = 60, 12, 512, 19, 5000
GOLD_SEEDS = (6, 7, 9)          # found by search: the margin conditions below hold (the generator asserts them)
MARGIN = 1e-3          # argmax gap, rank top / top + 1 gap, centre distance against 0.9
ORDER_MARGIN = 2e-4    # gaps between the ranks in between: they only order the appended ids; twice the fp32 bar at D = 512


def unpack_features(q8):
    """int8 -> fp32 features: the goldens store features as multiples of 1 / 16, a quarter of the bytes"""
    return q8.astype(np.float32) / np.float32(16.0)


def text_case(seed, K=GOLD_K, roots=GOLD_ROOTS, D=GOLD_D, Q=GOLD_Q, quantise=True):
    """One scene of the text query: leaf features with a shared part per coarse cluster, texts near one leaf each, occupancy
    counts that zero some leaves at both thresholds (2 and 5), leaf centres in blobs per coarse cluster so that some of the
    top-10 candidates lie within 0.9 of the best and some do not.  -> dict of arrays (features already fp32)."""
    rng = np.random.default_rng(seed)
    per = max(1, K // max(1, roots))
    root_of = np.minimum(np.arange(K) // per, max(1, roots) - 1)
    # features with a dozen strong directions, so that the similarities spread over tenths and ranks are tie-free by a margin
    L = min(12, D)
    basis = rng.standard_normal((L, D))
    root_lat = rng.standard_normal((max(1, roots), L))
    leaf_lat = 0.7 * root_lat[root_of] + rng.standard_normal((K, L))
    leaf = leaf_lat @ basis / np.sqrt(L) + 0.3 * rng.standard_normal((K, D))
    target = rng.integers(0, K, Q)
    text = (0.8 * leaf_lat[target] + rng.standard_normal((Q, L))) @ basis / np.sqrt(L) + 0.3 * rng.standard_normal((Q, D))
    if quantise:
        leaf = np.clip(np.round(leaf * 16), -127, 127).astype(np.int8)
        text = np.clip(np.round(text * 16), -127, 127).astype(np.int8)
        leaf_f, text_f = unpack_features(leaf), unpack_features(text)
    else:
        leaf_f, text_f = leaf.astype(np.float32), text.astype(np.float32)
        leaf, text = leaf_f, text_f
    occu = rng.integers(0, 25, K).astype(np.int64)
    blob = rng.uniform(-1.0, 1.0, (max(1, roots), 6))
    centers = np.concatenate([blob[root_of] + rng.normal(0, 0.22, (K, 6)), rng.uniform(-1, 1, (1, 6))]).astype(np.float32)
    return dict(text=text_f, leaf=leaf_f, text_q=text, leaf_q=leaf, occu=occu, centers=centers,
                leaf_num=np.float32(K / max(1, roots)))


MAX_LEAVES = 8192      # ogs_query_max_leaves(); the GPU test asserts that the library says the same
SHAPE_KS, SHAPE_DS, SHAPE_QS, SHAPE_TOP = (1, 9, 10, 11, 60, 640, MAX_LEAVES), (1, 6, 512, 513), (1, 21), 10
# of the 1 + 21 rows of every (K, D > 1), at least this many have every decision clear and are compared exactly: a third.
# A property of the seeded inputs, asserted on the CPU; the crowded ranks of 8192 leaves in six dimensions leave the fewest.
SHAPE_MIN_EXACT = 8


def shape_case(K, D, Q):
    """The similarity / selection input of one (K, D, Q) of the shape sweep: text_case (a fifth of the leaves zeroed by
    occupancy) with, at Q > 1, text row 2 zero (similarities exactly 0, best = leaf 0)."""
    c = text_case(300 + K + D + Q, K=K, roots=max(1, K // 5), D=D, Q=Q, quantise=False)
    if Q > 1:
        c["text"][2] = 0.0
    return c


def shape_decided(c, sim64, top=SHAPE_TOP, min_occu=5, all_exact=False):
    """rows of a shape_case whose `selected` / `count` are compared exactly (tests/query_restatement.decided_rows).
    `all_exact`: the similarities under test equal `sim64` bit for bit, so every tie is the same tie on both sides."""
    from tests import query_restatement as qr
    zeroed = np.ones(len(c["occu"]), bool) if all_exact else c["occu"] < min_occu
    return qr.decided_rows(sim64, zeroed, c["centers"], c["leaf_num"], top, MARGIN, ORDER_MARGIN)


def small_case():
    """K = 7 < top: all seven leaves are ranked, none is zeroed, every centre coincides and leaf_num admits every id, so
    `selected` is the whole rank order."""
    c = text_case(6, K=7, roots=1)
    return dict(c, centers=np.zeros((8, 6), np.float32), leaf_num=np.float32(7.0), occu=np.full(7, 9, np.int64))


def point_case(seed, K=GOLD_K, T=GOLD_Q, N=GOLD_N):
    """Points of the ScanNet evaluation: leaf ids with the dummy id K among them (clamped at K - 1), labels 0..T, an ignore
    mask.  The labels follow a fixed leaf -> class map most of the time, so that the IoUs are neither 0 nor 1."""
    rng = np.random.default_rng(1000 + seed)
    leaf_ind = rng.integers(0, K + 1, N).astype(np.int64)
    leaf_ind[rng.random(N) < 0.05] = K
    guess = (np.minimum(leaf_ind, K - 1) * 7) % T + 1
    gt = np.where(rng.random(N) < 0.6, guess, rng.integers(0, T + 1, N)).astype(np.int64)
    gt[rng.random(N) < 0.1] = 0
    return dict(leaf_ind=leaf_ind, gt=gt, ignore=rng.random(N) < 0.05)


def split_case(n, Q, K=37, seed=0, holes=True):
    """Inputs of the multi-split: leaf ids in [-1, K] (-1 and K belong to no group), a leaf table in which leaf 0 is in no
    group and leaf 1 in every group -- every one of the Q when `holes` is False, otherwise every one but groups 0, Q // 2 and
    Q - 1, which then stay empty (empty groups at both ends and in the middle) -- a row filter and a group filter."""
    rng = np.random.default_rng(50_000 + 131 * n + Q + seed)
    leaf_ind = rng.integers(-1, K + 1, n).astype(np.int64)
    words = [0] * K
    for k in range(2, K):
        for q in rng.choice(Q, size=min(Q, int(rng.integers(0, 4))), replace=False):
            words[k] |= 1 << int(q)
    words[1] = (1 << Q) - 1
    if holes:
        empty = (1 << 0) | (1 << (Q // 2)) | (1 << (Q - 1))
        words = [w & ~empty for w in words]
    words[0] = 0
    row_ok = rng.random(n) < 0.7
    group_keep = rng.random(Q) < 0.6
    return dict(leaf_ind=leaf_ind, words=np.array(words, dtype=np.uint64), K=K, row_ok=row_ok, group_keep=group_keep)


SCENE = dict(P=3000, W=96, H=64, f=70.0, seed=41, leaves=12)
# two queries that share leaf 4; leaf 10 holds about 60 Gaussians (under the 100 of better_vis, over the 10 of the last rule);
# an empty selection; leaf 11 holds 11 (two of them far from the rest: under 10 only after the kNN filter, which decides when
# better_vis is off); the dummy id 12 beside a real leaf
SCENE_SELECTIONS = [[4, 7], [4, 5], [10], [], [11], [12, 9]]


def query_scene():
    """The render_queries scene: raw parameters for tests/golden/render_cases.TinyModel, the camera, 12 leaves in four
    vertical bands (5 % of the points carry the dummy id 12), a pre-mask.  CPU torch tensors."""
    import torch
    from opengaussian_amd.synthetic import make_camera, make_scene
    P, W, H, f = SCENE["P"], SCENE["W"], SCENE["H"], SCENE["f"]
    sc = make_scene(P, W, H, f, f, seed=SCENE["seed"], log_scale_mean=-3.0)
    g = torch.Generator().manual_seed(9000 + SCENE["seed"])
    op = sc.opacities.clamp(1e-4, 1 - 1e-4)
    params = {
        "_xyz": sc.means3D.clone(), "_features_dc": sc.shs[:, :1].clone(), "_features_rest": sc.shs[:, 1:].clone(),
        "_scaling": torch.log(sc.scales), "_rotation": sc.rotations * (0.5 + torch.rand(P, 1, generator=g)),
        "_opacity": torch.log(op / (1 - op)), "_ins_feat": torch.randn(P, 6, generator=g),
    }
    x, y, z = sc.means3D.unbind(1)
    u, v = x / z.clamp_min(0.3) / (W / (2 * f)), y / z.clamp_min(0.3) / (H / (2 * f))
    band = ((u + 1.1) / 2.2 * 4).floor().clamp(0, 3).to(torch.int64)
    leaf = band * 3 + torch.randint(0, 3, (P,), generator=g)
    leaf[torch.rand(P, generator=g) < 0.05] = 12
    pre_mask = torch.rand(P, generator=g) < 0.8
    # rows that every filter of render() keeps with room to spare: well inside the frustum, small
    safe = (z > 2.5) & (u.abs() < 0.8) & (v.abs() < 0.8) & (sc.scales < 0.09).all(1)
    for lid, want in ((10, 60), (11, 11)):
        rows = torch.nonzero((leaf == lid) & safe).flatten()
        if lid == 11:                                          # nine neighbours and the two rows farthest from them
            d = (sc.means3D[rows] - sc.means3D[rows[0]]).norm(dim=1)
            near = torch.argsort(d)
            rows = torch.cat((rows[near[:9]], rows[near[-2:]]))
        else:
            rows = rows[:want]
        leaf[leaf == lid] = 9
        leaf[rows] = lid
        pre_mask[rows] = True
    return dict(params=params, cam=make_camera(W, H, f, f), leaf=leaf, pre_mask=pre_mask, scales=sc.scales,
                bg=torch.tensor([0.2, 0.1, 0.3]))


def planted_case(K, D, Q, seed=0, top=10):
    """Similarity inputs whose first `top` ranks are PLANTED: query q has `top` leaves of its own at cosines 0.95, 0.90, ...
    while every other leaf is random (|cosine| below 0.3 at D >= 512 with room to spare), so that best, ranked order and the
    cut after rank `top` all have margins far above MARGIN at any K >= Q * top.  Leaves 3 and 5 are zeroed by occupancy, text
    row 0 is zero.  Centres: the planted leaves of a query alternate between 0.5 and 1.5 from the best one's."""
    assert K >= Q * top and D >= 64
    rng = np.random.default_rng(7000 + K + D + Q + seed)
    leaf = rng.standard_normal((K, D))
    text = rng.standard_normal((Q, D))
    text /= np.linalg.norm(text, axis=1, keepdims=True)
    slots = rng.permutation(np.arange(6, K))[:Q * top].reshape(Q, top)          # never leaves 3 and 5
    centers = rng.uniform(-1, 1, (K + 1, 6)) * 10.0
    for q in range(Q):
        for r, k in enumerate(slots[q]):
            a = 0.95 - 0.05 * r
            noise = rng.standard_normal(D)
            noise -= noise @ text[q] * text[q]
            leaf[k] = (a * text[q] + np.sqrt(1 - a * a) * noise / np.linalg.norm(noise)) * rng.uniform(0.5, 2.0)
            off = np.zeros(6)
            off[r % 6] = 0.5 if r % 2 else 1.5
            centers[k] = centers[slots[q][0]] + (off if r else 0)
    text *= rng.uniform(0.5, 2.0, (Q, 1))
    text[0] = 0.0
    occu = np.full(K, 9, np.int64)
    occu[[3, 5]] = 1
    return dict(text=text.astype(np.float32), leaf=leaf.astype(np.float32), occu=occu, centers=centers.astype(np.float32),
                leaf_num=np.float32(K), slots=slots)
