"""CPU side of the attribution feature (`pmx_attribute`): the record's node -> atoms map, the NumPy restatement of
tests/attribution_ref.py against the reference's own numbers (tests/golden/attribution_<set>.npz, minted by
tests/golden/make_golden_attribution.py), atom shares, and the C entry point's argument checks."""

import ctypes
import json

import numpy as np
import pytest

from attribution_ref import attribution
from conftest import GOLDEN, load_golden
from explain_ref import NONE, Tables

ATTRIBUTION_SETS = ("set_6oim_c8", "set_6oim_c1", "set_6oim_c64", "set_c21_c8", "set_6oim_c8_weights", "set_s64_c8")


def load_mols(name):
    """The feature molecules a golden set's library was packed from (`<set>_mols.npz`, written by tests/golden/make_golden.py)."""
    from pharmaconet_amd.library import LigandFeatures

    d = np.load(GOLDEN / f"{name}_mols.npz")
    mols, o = [], 0
    for t, shp in zip(json.loads(str(d["topology"])), d["shapes"]):
        cnt = int(np.prod(shp))
        feats = [(f[0], f[1] if isinstance(f[1], int) else tuple(f[1]), f[2] if isinstance(f[2], int) else tuple(f[2])) for f in t["features"]]
        mols.append(LigandFeatures(t["z"], t["nbrs"], feats, d["positions"][o : o + cnt].reshape(tuple(int(x) for x in shp))))
        o += cnt
    return mols


def attribution_rows(x):
    """Per fixture ligand: (library index, conformer, key [nl] with -1 for None, levels [nl], entry [nl, nl], node [64], total)."""
    for r, i in enumerate(x["index"]):
        lv = x["levels"][r]
        nl = int(np.count_nonzero(lv != 0xFE))
        key = x["key"][r, :nl].astype(np.int64)
        key[key == 0xFF] = NONE
        yield int(i), int(x["conformer"][r]), key, lv[:nl].astype(np.int64), x["entry"][r, :nl, :nl], x["node"][r], float(x["total"][r])


@pytest.mark.parametrize("name", ("set_6oim_c8", "set_c21_c8"))
def test_record_node_atoms_follows_the_packed_record(name):
    """The library of a golden set was packed from the reference's own LigandGraph: node count and, node by node, the type mask of the
    features on exactly that node's atoms must be the record's."""
    from pharmaconet_amd.constants import TYPE_ID
    from pharmaconet_amd.library import cluster_ligand, record_node_atoms

    _, lib, _, _ = load_golden(name)
    mols = load_mols(name)
    assert len(mols) == len(lib)
    seen = 0
    for i, mol in enumerate(mols):
        rec = lib.unpack(i)
        if rec["n_conf"] == 0:
            continue  # (a marker record: the molecule is outside the engine's limits)
        atoms = record_node_atoms(mol)
        assert len(atoms) == rec["n_nodes"] == len(cluster_ligand(mol).typemask)
        by_atoms = {}
        for ftype, a, _ in mol.features:
            k = (a,) if isinstance(a, int) else tuple(sorted(a))
            by_atoms[k] = by_atoms.get(k, 0) | 1 << TYPE_ID[ftype]
        for u, at in enumerate(atoms):
            assert at == tuple(sorted(at)) and all(0 <= a < mol.num_atoms for a in at)
            tm = int(rec["typemask"][u])
            assert tm & ~by_atoms[at] == 0, (i, u)
            if atoms.count(at) == 1:  # (an int and a 1-tuple of the same atom are two nodes: ligand.py:137)
                assert tm == by_atoms[at], (i, u)
        seen += len(atoms)
    assert seen > 0


@pytest.mark.parametrize("name", ATTRIBUTION_SETS)
def test_restatement_reproduces_the_reference(name):
    """Entries, node shares and total of the restatement against the reference's own (float32 sums, so 2e-6 of the leaf's total, the bar of
    the explain tests; exact zeros where the reference has none)."""
    from pharmaconet_amd.constants import weights_vector

    model, lib, weights, _ = load_golden(name)
    x = np.load(GOLDEN / f"attribution_{name}.npz")
    w7 = weights_vector(weights)
    n = 0
    for i, c, key, lv, entry, node, total in attribution_rows(x):
        rec = lib.unpack(i)
        out = attribution(model, rec, w7, lv, key, c, Tables(model, rec, w7))
        assert out["valid"], (name, i)
        bar = 2e-6 * total
        assert abs(out["total"] - total) <= bar, (name, i, out["total"], total)
        assert np.abs(out["entry"] - entry).max(initial=0.0) <= bar, (name, i)
        k = int(rec["n_nodes"])
        assert np.abs(out["node"] - node[:k]).max(initial=0.0) <= bar and (node[k:] == 0).all(), (name, i)
        assert abs(out["node"].sum() - total) <= 2 * bar
        n += total > 0
    assert n > 0


def test_atom_scores_share_a_node_among_its_atoms():
    from pharmaconet_amd.engine import Attribution
    from pharmaconet_amd.library import record_node_atoms

    mol = next(m for m in load_mols("set_6oim_c8") if any(len(a) > 1 for a in record_node_atoms(m)))
    atoms = record_node_atoms(mol)
    node = np.random.default_rng(5).uniform(0.0, 3.0, len(atoms))
    at = Attribution(indices=np.array([0]), conformers=np.array([0]), total=np.array([node.sum()]), node=[node], entry=[np.zeros((0, 0))],
                     fails=[np.zeros((0, 0), np.int64)], levels=[np.zeros(0, np.int64)], status=np.array([0], np.int32))
    sc = at.atom_scores(0, mol)
    assert sc.shape == (mol.num_atoms,)
    assert abs(sc.sum() - at.total[0]) <= 4 * len(atoms) * np.spacing(at.total[0])
    u = next(u for u, a in enumerate(atoms) if len(a) > 1)
    others = sum(node[v] / len(atoms[v]) for v in range(len(atoms)) if v != u and atoms[u][0] in atoms[v])
    assert abs(sc[atoms[u][0]] - (node[u] / len(atoms[u]) + others)) <= 1e-12
    with pytest.raises(ValueError):
        Attribution(at.indices, at.conformers, at.total, [node[:-1]], at.entry, at.fails, at.levels, at.status).atom_scores(0, mol)


def test_pmx_attribute_checks_its_arguments_without_a_gpu():
    import __graft_entry__ as entry

    entry.build()
    from pharmaconet_amd import _ffi

    lib = _ffi.load()
    none = [None] * 6
    assert lib.pmx_attribute(None, None, None, None, None, None, 1, *none, None) == 1 and b"null" in lib.pmx_last_error()
    fake = ctypes.create_string_buffer(256)  # (stands for a model and a library: neither call below gets as far as reading one)
    w = (ctypes.c_float * _ffi.NUM_TYPES)(*([1.0] * _ffi.NUM_TYPES))
    addr = ctypes.addressof(fake)
    assert lib.pmx_attribute(addr, addr, w, None, None, None, 0, *none, None) == 0  # n = 0 succeeds
    assert lib.pmx_attribute(addr, addr, w, None, None, None, 65537, *none, None) == 1 and b"65536" in lib.pmx_last_error()
    assert lib.pmx_attribute(addr, addr, w, None, None, None, 1, *none, None) == 1 and b"null" in lib.pmx_last_error()
