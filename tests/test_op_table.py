"""CPU: the operator ids are said once per language and the sayings agree -- the two enums of include/tmlqcd_hip.h, the rows of
tmlqcd_amd/csrc/op_table.h (one per id, under the reference's function name) and the two maps of tmlqcd_amd/hip.py, with the four
dictionaries the solvers' wrappers index derived from them."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what the four dictionaries held as literals before they were derived (tests/test_bicg_abi.py and tests/test_ndsw_abi.py pin two of them too)
OPS = {"Qtm_pm_psi": 0, "Qtm_plus_psi": 1, "Qtm_minus_psi": 2, "Mtm_plus_psi": 3, "Mtm_minus_psi": 4, "Qsw_pm_psi": 5}
MMS_OPS = {"Qtm_pm_psi": 0, "Qsw_pm_psi": 5, "Q_pm_psi": 6}
BICG_OPS = {"Qtm_plus_psi": 1, "Qtm_minus_psi": 2, "Mtm_plus_psi": 3, "Mtm_minus_psi": 4, "Mtm_plus_sym_psi": 7, "Mtm_minus_sym_psi": 8,
            "Qsw_plus_psi": 9, "Qsw_minus_psi": 10, "Msw_plus_psi": 11, "D_psi": 12}
ND_OPS = {"Qtm_pm_ndpsi": 0, "Qsw_pm_ndpsi": 1}


def _enum(prefix):
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_hip.h")).read()
    return {n: int(v) for n, v in re.findall(r"\b%s([A-Z0-9_]+)\s*=\s*(\d+)" % prefix, hdr)}


def _rows(macro):
    """the rows of one X-macro list of op_table.h: [(id suffix, reference function, fields, clover, fp32, solvers)]"""
    lines = open(os.path.join(ROOT, "tmlqcd_amd", "csrc", "op_table.h")).read().splitlines()
    i = next(k for k, l in enumerate(lines) if l.startswith("#define %s(X)" % macro))
    text = []
    while lines[i].rstrip().endswith("\\"):      # the definition ends with the first line without a continuation
        i += 1
        text.append(lines[i])
    return [tuple(c.strip() for c in r.split(",")) for r in re.findall(r"\bX\(([^)]*)\)", "\n".join(text))]


def test_both_enums_are_dense_and_every_id_has_one_row():
    for prefix, macro, n in (("TMHIP_OP_", "TMHIP_OP_TABLE", 13), ("TMHIP_ND_OP_", "TMHIP_ND_OP_TABLE", 2)):
        ids, rows = _enum(prefix), _rows(macro)
        assert sorted(ids.values()) == list(range(n)), prefix
        assert sorted(r[0] for r in rows) == sorted(ids), macro
        assert all(len(r) == 6 for r in rows), macro
        assert len({r[1] for r in rows}) == n, macro


def test_python_maps_equal_the_enums_name_for_name():
    import tmlqcd_amd.hip as h
    ids, nd = _enum("TMHIP_OP_"), _enum("TMHIP_ND_OP_")
    assert h.ALL_OPS == {name: ids[suffix] for suffix, name, *_ in _rows("TMHIP_OP_TABLE")}
    assert h.ND_OPS == {name: nd[suffix] for suffix, name, *_ in _rows("TMHIP_ND_OP_TABLE")}


def test_derived_dictionaries_equal_their_former_literals():
    import tmlqcd_amd.hip as h
    assert h.OPS == OPS
    assert h.MMS_OPS == MMS_OPS
    assert h.BICG_OPS == BICG_OPS
    assert h.ND_OPS == ND_OPS
    for d in (h.OPS, h.MMS_OPS, h.BICG_OPS):
        assert all(h.ALL_OPS[k] == v for k, v in d.items())


def test_table_columns_say_what_the_dictionaries_say():
    rows = {r[1]: r for r in _rows("TMHIP_OP_TABLE")}
    for bit, names in (("TMHIP_S_CG", OPS), ("TMHIP_S_MMS", MMS_OPS), ("TMHIP_S_BICG", BICG_OPS), ("TMHIP_S_RATCOR", ("Qtm_pm_psi", "Qsw_pm_psi"))):
        assert {n for n, r in rows.items() if bit in r[5].split(" | ")} == set(names), bit
    assert {n for n, r in rows.items() if r[2] == "FULL"} == {"Q_pm_psi", "D_psi"}
    assert {n for n, r in rows.items() if r[3] != "NONE"} == {"Qsw_pm_psi", "Qsw_plus_psi", "Qsw_minus_psi", "Msw_plus_psi"}
    assert rows["Qsw_minus_psi"][3] == "TERM_MINUS_MU"
    assert {n for n, r in rows.items() if r[4] == "1"} == {"Qtm_pm_psi", "Qsw_pm_psi"}      # the mixed solvers' set
    nd = {r[1]: r for r in _rows("TMHIP_ND_OP_TABLE")}
    assert {n: (r[2], r[3], r[5]) for n, r in nd.items()} == {"Qtm_pm_ndpsi": ("EO", "NONE", "TMHIP_S_ND"), "Qsw_pm_ndpsi": ("EO", "TERM", "TMHIP_S_ND")}
