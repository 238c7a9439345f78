"""Multi-bank counting, the part that needs no GPU: the binding's surface (gkc.Banks, GKC_SOLIDITY_*, the gkc_banks_* exports) and the numpy statement of the
reference's solidity kinds (CountProcessorSolidity.hpp:176-304) that tests/test_gpu_banks.py checks the device against — here checked itself against the
answers the reference's own unit test records (TestDSK.cpp:482-612, tests/golden/perbank_kinds.json)."""
import json
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
from tests.util import naive_counts

KINDS = ("sum", "min", "max", "one", "all", "custom")


def solid_mask(vectors, kind, amin, amax, solid_vec=None):
    """vectors int32[n][nb_banks] -> bool[n]: CountProcessorSolidity*::check for every row. amin / amax: one closed range for all banks or one per bank;
    sum / min / max look at range 0 only (_thresholds[0]); custom: bank i is inside its range exactly when solid_vec[i]"""
    v = np.asarray(vectors, dtype=np.int64)
    assert v.ndim == 2
    nb = v.shape[1]
    lo = np.broadcast_to(np.asarray(amin, dtype=np.int64), (nb,))
    hi = np.broadcast_to(np.asarray(amax, dtype=np.int64), (nb,))
    inside = (v >= lo[None, :]) & (v <= hi[None, :])
    if kind == "sum":
        s = v.sum(axis=1); return (s >= lo[0]) & (s <= hi[0])
    if kind == "min":
        s = v.min(axis=1); return (s >= lo[0]) & (s <= hi[0])
    if kind == "max":
        s = v.max(axis=1); return (s >= lo[0]) & (s <= hi[0])
    if kind == "one":
        return inside.any(axis=1)
    if kind == "all":
        return inside.all(axis=1)
    if kind == "custom":
        sv = np.asarray(solid_vec).astype(bool)
        assert sv.shape == (nb,)
        return (inside == sv[None, :]).all(axis=1)
    raise ValueError(kind)


def fixture_cases(golden_dir):
    """-> [(table name, sequences, k, [(kind, amin, amax, recorded number of solid k-mers), ...]), ...]"""
    fx = json.load(open(os.path.join(golden_dir, "perbank_kinds.json")))
    vec = json.load(open(os.path.join(golden_dir, "reference_unit_vectors.json")))
    out = []
    for name in ("perbank1", "perbank2"):
        t = fx[name]; cols = t["columns"]; cases = []
        for row in t["rows"]:
            r = dict(zip(cols, row))
            amax = r.get("amax", t.get("amax"))
            cases += [(kind, r["amin"], amax, r[kind]) for kind in KINDS if kind in r]
        out.append((name, vec[t["vectors"]]["seqs"], t["k"], cases))
    return out


def naive_vectors(seqs, k):
    """one bank per sequence -> (sorted k-mers, int32[n][len(seqs)])"""
    per = [naive_counts([s], k) for s in seqs]
    keys = sorted(set().union(*per))
    return keys, np.array([[p.get(x, 0) for p in per] for x in keys], dtype=np.int32).reshape(len(keys), len(seqs))


@pytest.fixture(scope="module")
def gkc():
    ge.build()
    return ge.load().gkc


def test_fixture_holds_every_recorded_row(golden_dir):
    cases = fixture_cases(golden_dir)
    assert [(n, len(c)) for n, _, _, c in cases] == [("perbank1", 9), ("perbank2", 45)]
    # the sum columns are the rows tests/test_oracle_golden.py already uses
    vec = json.load(open(os.path.join(golden_dir, "reference_unit_vectors.json")))
    assert [[a, n] for kind, a, _, n in cases[0][3] if kind == "sum"] == vec["dsk_perbank1"]["sum_cases"]
    assert [[a, b, n] for kind, a, b, n in cases[1][3] if kind == "sum"] == vec["dsk_perbank2"]["sum_cases"]


def test_solid_mask_reproduces_the_reference_answers(golden_dir):
    for name, seqs, k, cases in fixture_cases(golden_dir):
        keys, vectors = naive_vectors(seqs, k)
        for kind, amin, amax, recorded in cases:
            assert int(solid_mask(vectors, kind, amin, amax).sum()) == recorded, (name, kind, amin, amax)
    # the occurrence table in the reference's comment (TestDSK.cpp: DSK_perBank2)
    keys, vectors = naive_vectors(fixture_cases(golden_dir)[1][1], 5)
    rows = sorted(tuple(r) for r in vectors.tolist() if sum(r) > 1)
    assert rows == [(0, 2, 0), (1, 1, 0), (2, 1, 2)] and len(keys) == 15


def test_solid_mask_custom_and_per_bank_ranges():
    v = np.array([[0, 0], [1, 0], [0, 3], [2, 2], [5, 1]], np.int32)
    assert solid_mask(v, "custom", 1, 9, [1, 0]).tolist() == [False, True, False, False, False]
    assert solid_mask(v, "custom", 1, 9, [1, 1]).tolist() == solid_mask(v, "all", 1, 9).tolist()
    assert solid_mask(v, "all", [1, 2], [9, 3]).tolist() == [False, False, False, True, False]
    assert solid_mask(v, "one", [4, 3], [9, 3]).tolist() == [False, False, True, False, True]
    assert solid_mask(v, "sum", [4, 100], [9, 100]).tolist() == [False, False, False, True, True]      # range 0 only


def test_binding_has_the_banks_surface(gkc):
    assert [gkc.GKC_SOLIDITY_SUM, gkc.GKC_SOLIDITY_MIN, gkc.GKC_SOLIDITY_MAX, gkc.GKC_SOLIDITY_ONE, gkc.GKC_SOLIDITY_ALL, gkc.GKC_SOLIDITY_CUSTOM] == list(range(6))
    hdr = open(os.path.join(ge.ROOT, "include", "gkc.h")).read()
    for i, name in enumerate(("SUM", "MIN", "MAX", "ONE", "ALL", "CUSTOM")):
        assert re.search(r"#define\s+GKC_SOLIDITY_%s\s+%d\b" % (name, i), hdr), name
    for meth in ("add", "evaluate", "partition_info", "partition", "vectors", "histogram", "all_counts", "close"):
        assert callable(getattr(gkc.Banks, meth)), meth
    assert callable(gkc.Counter.count_banks)
    assert gkc.Banks.TILE >= 64 and gkc.Banks.SCAN_BLOCK >= 64


def test_every_declared_banks_export_resolves(gkc):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ge.ROOT, "include", "gkc.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(gkc_banks_[a-z0-9_]+)\s*\(", hdr)))
    assert names == sorted(["gkc_banks_create", "gkc_banks_destroy", "gkc_banks_add", "gkc_banks_evaluate", "gkc_banks_partition_info", "gkc_banks_partition_counts",
                            "gkc_banks_partition_vectors", "gkc_banks_partition_counts_device", "gkc_banks_histogram"])
    L = gkc.lib()
    for n in names:
        assert n in gkc.SYMBOLS, n
        f = getattr(L, n)
        assert f.argtypes is not None, n


def test_binding_geometry_is_the_kernels(gkc):
    """Banks.TILE / Banks.SCAN_BLOCK (what tests/test_gpu_banks.py sizes its boundary cases from) are the constants of csrc/gkc_banks.hip"""
    src = open(os.path.join(ge.ROOT, "gatb-core_amd", "csrc", "gkc_banks.hip")).read()
    threads, per = map(int, re.search(r"BK_THREADS = (\d+), BK_PER_THREAD = (\d+);", src).groups())
    assert re.search(r"BK_TILE = BK_THREADS \* BK_PER_THREAD;", src)
    assert gkc.Banks.TILE == threads * per
    assert gkc.Banks.SCAN_BLOCK == int(re.search(r"BK_SCAN_BLOCK = (\d+);", src).group(1))
