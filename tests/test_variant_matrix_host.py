"""The matrix of tests/variant_matrix.py without a GPU: the union of its rows' claims is exactly what the library's tables hold
(rt_debug_variant_tables: 66 k_shade, 66 k_intersect, 15 k_debug_bounce keys, the seven closest-hit kernels outside the tables), and every
row's reference — the oracle and the numpy restatements alone — meets the coverage conditions that keep the row from passing emptily."""
import pytest

import variant_matrix as vm


def test_the_rows_claim_exactly_the_tables(rt):
    tables = rt.variant_tables()
    assert (len(tables["shade"]), len(tables["intersect"]), len(tables["debug_bounce"]), len(tables["untabled"])) == (66, 66, 15, 7)
    union = {family: set() for family in tables}
    for row in vm.ROWS:
        for family, keys in vm.claims(rt, row).items():
            union[family] |= keys
    for family in ("shade", "intersect", "debug_bounce"):
        assert not vm.UNREACHABLE[family] & tables[family], "a key listed as unreachable still has a kernel"
    spell = lambda keys: sorted(" ".join(k) if isinstance(k, tuple) and k else (k or "no flag") for k in keys)
    for family in tables:
        assert not tables[family] - union[family], (family, "no row claims", spell(tables[family] - union[family]))
        assert not union[family] - tables[family], (family, "claimed without a kernel", spell(union[family] - tables[family]))


def test_the_flag_names_come_from_the_library(rt):
    f = rt._ffi
    assert len(rt.variant_flag_names(f.FAMILY_SHADE)) == 8 and len(rt.variant_flag_names(f.FAMILY_INTERSECT)) == 8
    assert rt.variant_flag_names(f.FAMILY_DEBUG_BOUNCE) == ("MOTION", "PLANAR", "LIGHTS") and len(rt.variant_flag_names(f.FAMILY_UNTABLED)) == 7
    with pytest.raises(rt.RtError):
        rt.variant_flag_names(9)


def test_row_names_are_unique():
    assert len(set(vm.ROW_NAMES)) == len(vm.ROWS)


@pytest.mark.parametrize("name", vm.ROW_NAMES)
def test_the_reference_of_a_row_covers_what_the_row_exists_for(rt, orc, name):
    row = vm.ROWS[vm.ROW_NAMES.index(name)]
    X = vm.expected(rt, orc, row)
    print(name, X["stats"])
    vm.check_coverage(row, X["stats"])
    if row["grid"] and "motion" not in row["sets"]:  # the grid the static scene gets: one cell high, or several (with movers: the GPU test's ledger says)
        g = rt.grid_build(X["B"]["scene"])
        assert g is not None and (g["dims"][1] == 1) == (row["grid"] == "flat"), g and g["dims"]
