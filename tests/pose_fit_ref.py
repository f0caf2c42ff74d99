"""NumPy restatement of `pmx_pose_fit` (the comment of include/pmx.h): one row at a time, float64 with every operation rounded in the order
the header gives. NumPy's `a * b + c` on float64 is two rounded operations (no fused multiply-add) and the division is correctly rounded;
`np.exp` is the C library's, within an ulp of the device's. A node's sums run in a plain loop in ascending model node, and the row's four
sums go through the same butterfly of 64 lanes as the kernel's, so the only difference between the two is the exp.

Key-mode pairs come from tests/align_ref.py's `pair_list` (on tests/explain_ref.py's `Tables`), the restatement of `pmx_align`'s.

Also here: the seeded free-mode cases the CPU and the GPU tests share (`free_case`), so that the CPU test can assert their margins."""

from __future__ import annotations

from functools import lru_cache

import numpy as np

import align_ref
from clash_ref import pose
from explain_ref import NONE, Tables, candidates

OK, UNSUPPORTED, KEY_INVALID = 0, 1, 4
WORDS, MAX_NODES, MAX_MODEL_NODES = 4, 64, 256


def wave_sum(values) -> float:
    """The fixed butterfly of pmx_pose.h over 64 lanes: at step k lanes i and i ^ k both form v_i + v_(i ^ k)."""
    v = np.zeros(64, dtype=np.float64)
    v[: len(values)] = values
    lanes = np.arange(64)
    for k in (1, 2, 4, 8, 16, 32):
        v = v + v[lanes ^ k]
    return float(v[0])


def _invalid(n: int, nm: int, status: int) -> dict:
    return dict(status=status, summary=np.full(4, np.nan), count=np.zeros(4, np.int64), node_fit=np.full(n, np.nan), node_best=np.full(n, np.nan),
                node_z2=np.full(n, np.nan), node_target=np.full(n, -1, np.int64), hotspot_z2=np.full(nm, np.nan), hotspot_node=np.full(nm, -1, np.int64),
                fingerprint=np.zeros(WORDS, np.uint64), margin=np.inf, pairs=[])


def key_pairs(model, rec, w7, levels, key, c: int):
    """None when (c, key) is not valid for the record as `pmx_align` sees it; else {u: [m ascending]} of the key's pairs (weights not yet
    looked at: `fit_row` leaves out what has no weight or no sigma, as it does in free mode)."""
    T = Tables(model, rec, w7)
    nl = len(levels)
    key = [int(k) for k in key] + [NONE] * (nl - len(key))
    valid = 0 <= c < T.C and all(k == NONE for k in key[nl:])
    valid = valid and all(key[l] == NONE or key[l] in candidates(model, rec, int(levels[l])) for l in range(nl))
    if not valid:
        return None
    ones = np.ones(7)  # (every pair: pair_list drops weights <= 0, which fit_row does itself)
    return {u: list(ms) for u, _, ms, _ in align_ref.pair_list(model, Tables(model, rec, ones), levels, key[:nl], c)}


def free_pairs(node_type, rec) -> dict:
    """{u: [m ascending]}: every node of the record with every model node whose type is in its type mask."""
    out = {}
    for u in range(int(rec["n_nodes"])):
        tm = int(rec["typemask"][u])
        ms = [m for m in range(len(node_type)) if (tm >> int(node_type[m])) & 1]
        if ms:
            out[u] = ms
    return out


def fit_row(node_type, centers, sigmas, w7, rec, c: int, R, t, pairs="free") -> dict:
    """One row. `rec`: the unpacked record, or None for an index outside the library. `pairs`: "free", or what `key_pairs` returned (None:
    the key is not valid). Returns status, summary [4], count [4], the per-node arrays cut to the record's n, the per-hotspot arrays cut to
    Nm, the fingerprint (uint64 [4]), `pairs` [(u, m, z2, passes)] and `margin`: the smallest |d2 - 4 v| / (4 v) over the pairs, and the
    smallest relative gap between the best and the second-best z2 of a node, and of a hotspot (two z2 of the same bits are no gap: both
    sides take the lower index) - how far the row's integers are from changing."""
    nm = len(node_type)
    node_type = np.asarray(node_type, dtype=np.int64)
    Y = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    S = np.asarray(sigmas, dtype=np.float64).reshape(-1)
    assert len(Y) == nm and len(S) == nm
    w = np.asarray(w7, dtype=np.float32).astype(np.float64)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    if rec is None or not (1 <= int(rec["n_conf"]) <= 64):
        return _invalid(0, nm, UNSUPPORTED)
    n = int(rec["n_nodes"])
    if not (0 <= c < int(rec["n_conf"])) or not (np.isfinite(R).all() and np.isfinite(t).all()) or pairs is None:
        return _invalid(n, nm, KEY_INVALID)
    targets = free_pairs(node_type, rec) if isinstance(pairs, str) else pairs
    p = pose(rec["xyz"][:, :, c], R, t)  # [n, 3]
    node_fit, node_best, node_z2, node_target = np.full(n, -1.0), np.full(n, -1.0), np.full(n, -1.0), np.full(n, -1, np.int64)
    hz2, hnode = np.full(nm, np.inf), np.full(nm, -1, np.int64)
    lane_fit, lane_ideal, lane_best, lane_bw = np.zeros(64), np.zeros(64), np.zeros(64), np.zeros(64)
    bits = np.zeros(MAX_MODEL_NODES, np.uint8)
    count = np.zeros(4, np.int64)
    margin = np.inf
    listed = []
    per_hotspot = {}
    for u in range(n):
        sum_g = sum_w = 0.0
        n_u = pass_u = 0
        best = None
        z2s = []
        for m in targets.get(u, []):
            wm, s = float(w[node_type[m]]), float(S[m])
            if not wm > 0.0 or not (np.isfinite(s) and s > 0.0):
                continue
            e = p[u] - Y[m]
            d2 = float((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
            v = s * s
            z2 = d2 / v
            passes = d2 < 4.0 * v
            g = wm * float(np.exp(-0.5 * z2))
            sum_g = sum_g + g
            sum_w = sum_w + wm
            n_u += 1
            pass_u += int(passes)
            if best is None or z2 < best[0]:
                best = (z2, m, g, wm)
            z2s.append(z2)
            per_hotspot.setdefault(m, []).append((z2, u))
            if passes:
                bits[m] = 1
            margin = min(margin, abs(d2 - 4.0 * v) / (4.0 * v))
            listed.append((u, m, z2, passes))
        if n_u == 0:
            continue
        node_fit[u], node_z2[u], node_target[u], node_best[u] = sum_g / float(n_u), best[0], best[1], best[2]
        lane_fit[u], lane_ideal[u], lane_best[u], lane_bw[u] = node_fit[u], sum_w / float(n_u), best[2], best[3]
        count += (1, n_u, int(2 * pass_u >= n_u), pass_u)
        margin = min(margin, _gap(z2s))
    for m, zs in per_hotspot.items():
        hz2[m], hnode[m] = min(zs)  # (the smallest z2, then the lowest u)
        margin = min(margin, _gap([z for z, _ in zs]))
    summary = np.array([wave_sum(lane_fit), wave_sum(lane_ideal), wave_sum(lane_best), wave_sum(lane_bw)])
    return dict(status=OK, summary=summary, count=count, node_fit=node_fit, node_best=node_best, node_z2=node_z2, node_target=node_target, hotspot_z2=hz2,
                hotspot_node=hnode, fingerprint=np.packbits(bits, bitorder="little").view(np.uint64).copy(), margin=float(margin), pairs=listed)


def _gap(z2s) -> float:
    """The relative gap between the smallest and the next distinct value (inf with fewer than two distinct values)."""
    zs = sorted(set(z2s))
    return (zs[1] - zs[0]) / zs[1] if len(zs) > 1 else np.inf


# ------------------------------------------------------------------------------------------------------------ the shared free-mode cases
NODE_COUNTS = (1, 2, 63, 64)
FREE_CASES = ((1, 8), (37, 1), (63, 64), (64, 8), (65, 1), (110, 8), (222, 64))  # (model nodes, conformer stride): every count and every stride
ROWS = 97


def sized_model(nm: int):
    """(model, node types, centers [nm, 3], sigmas [nm], weights dict, override): a model of `nm` nodes. 37 and 110 are the 6OIM and the
    110-node fixture models as they are (override False: their own centres and radii). Every other size is the 6OIM model enlarged
    (test_gpu_hotspots.enlarged) and cut to its first nm nodes, clusters that lose all their nodes dropped, with the centres and radii tiled,
    copy k shifted by 0.3 k A in x and its radii widened by 0.05 k: what `centers=` / `sigmas=` are for."""
    from conftest import load_golden

    if nm in (37, 110):
        model, _, weights, _ = load_golden("set_6oim_c8" if nm == 37 else "set_l110_c8")
        assert model.num_nodes == nm
        return model, np.asarray(model.flat.node_type), model.node_centers, model.node_radii, weights, False
    from pharmaconet_amd import PharmacophoreModel
    from pharmaconet_amd.pharmacophore_model import FlatModel, _node_masks, cluster_node_sets
    from test_gpu_hotspots import enlarged

    base, _, weights, _ = load_golden("set_6oim_c8")
    n0 = base.num_nodes
    copies = -(-nm // n0)
    flat = enlarged(base, copies).flat
    masks = [mask & ((1 << nm) - 1) for mask in cluster_node_sets(flat)]
    keep = [a for a, mask in enumerate(masks) if mask]
    cut = PharmacophoreModel()
    cut._state = base._state
    cut._flat = FlatModel(node_type=flat.node_type[:nm].copy(), edge_mean=np.ascontiguousarray(flat.edge_mean[:nm, :nm]), edge_std=np.ascontiguousarray(flat.edge_std[:nm, :nm]),
                          cluster_nodes=_node_masks([masks[a] for a in keep], nm), cluster_typemask=flat.cluster_typemask[keep], cluster_center=flat.cluster_center[keep],
                          cluster_size=flat.cluster_size[keep], cluster_type=tuple(flat.cluster_type[a] for a in keep))
    k = np.repeat(np.arange(copies), n0)[:nm]
    centers = np.tile(base.node_centers, (copies, 1))[:nm] + 0.3 * k[:, None] * np.array([1.0, 0.0, 0.0])
    sigmas = np.tile(base.node_radii, copies)[:nm] + 0.05 * k
    return cut, np.asarray(cut.flat.node_type), centers, sigmas, weights, True


@lru_cache(maxsize=None)
def free_case(nm: int, stride: int, seed: int = 0) -> dict:
    """One seeded free-mode call: a model of `nm` nodes, a library of 12 hand-made records of `stride` conformers - 1, 2, 63 and 64 nodes
    among them - and 97 rows (record, conformer) under random proper rotations and translations. A (record, conformer) has one motion, and
    its float32 coordinates are points near model nodes of a type the node has (a normal offset of 1.2 sigma) taken back through that
    motion: about half the nodes land within 2 sigma of something. Rows, restatement and all: computed once, shared, never written to."""
    from ligand_fp_ref import make_record
    from pharmaconet_amd import PackedLibrary
    from pharmaconet_amd.constants import weights_vector
    from test_gpu_clash import random_rotations

    model, node_type, centers, sigmas, weights, override = sized_model(nm)
    rng = np.random.default_rng(7919 * nm + 31 * stride + seed)
    counts = list(NODE_COUNTS) + [int(v) for v in rng.integers(3, 41, size=8)]
    records, motions = [], []
    for n in counts:
        R, t = random_rotations(rng, stride), rng.uniform(-15, 15, size=(stride, 3))
        masks = np.where(rng.random(n) < 0.5, 1 << rng.integers(0, 7, size=n), rng.integers(1, 128, size=n)).astype(np.uint8)  # (half of them of one type)
        own = [np.flatnonzero((int(mask) >> node_type.astype(np.int64)) & 1) for mask in masks]  # the model nodes a node pairs with (any, where it has none)
        near = np.stack([rng.choice(o if len(o) else np.arange(nm), size=stride) for o in own])
        y = centers[near] + 1.2 * sigmas[near][..., None] * rng.normal(size=(n, stride, 3))  # [n, C, 3], the pocket's frame
        x = np.einsum("cji,ncj->nci", R, y - t[None])  # x = R^T (y - t)
        records.append(make_record(masks, x.astype(np.float32)))
        motions.append((R, t))
    lib = PackedLibrary.from_records(records)
    idx = rng.integers(0, len(counts), size=ROWS)
    idx[: len(counts)] = np.arange(len(counts))  # (every record at least once)
    conf = rng.integers(0, stride, size=ROWS)
    rot = np.stack([motions[i][0][c] for i, c in zip(idx, conf)])
    trans = np.stack([motions[i][1][c] for i, c in zip(idx, conf)])
    w7 = weights_vector(weights)
    ref = [fit_row(node_type, centers, sigmas, w7, lib.unpack(int(i)), int(c), rot[r], trans[r]) for r, (i, c) in enumerate(zip(idx, conf))]
    return dict(model=model, lib=lib, weights=weights, w7=w7, node_type=node_type, centers=centers, sigmas=sigmas, override=override, indices=idx, conformers=conf, rotation=rot,
                translation=trans, ref=ref, counts=counts)
