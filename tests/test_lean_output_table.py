"""not-gpu: the table of the lean launches' outputs (libdwbc_amd/csrc/dwbc_fields.h, read through dwbc_lean_output_describe) against the names,
enumerators, element types and shapes the Python layer carried by hand before the table existed (GRAV_OUTPUTS / LINK_QUERY_OUTPUTS /
DYNAMICS_OUTPUTS / CONTACT_SPACE_OUTPUTS and the four _xxx_shape methods of libdwbc_amd/batch.py), written out below as the pin; the
output enums of include/dwbc_batch.h; and the Python layer, which must no longer keep a copy of its own.

Mutation tried: with the rows of "B" and "G" swapped in the dynamics block the library does not compile (the static_assert that ties row
i to enumerator i and slot i); with their names alone swapped it builds, and test_describe_reproduces_the_frozen_table (both sizes),
test_one_row_per_enumerator and test_python_keeps_no_copy fail."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import cases

ROOT = cases.ROOT
F64, I32 = np.float64, np.int32
# (n, n_queried): two sets, so that n / m = n - 6 and the query's length cannot be mistaken for each other or for a constant
DIMS = [(39, 1), (37, 16)]
FAMILIES = ("grav", "link_query", "dynamics", "contact_space")  # enum dwbc_lean_family
ENUMS = {"grav": ("dwbc_grav_output", "DWBC_GRAV_"), "link_query": ("dwbc_link_query_output", "DWBC_LQ_"),
         "dynamics": ("dwbc_dynamics_output", "DWBC_DYN_"), "contact_space": ("dwbc_contact_space_output", "DWBC_CS_")}


def _expected(n, q):
    """family -> [(name, enumerator, element type, per-instance shape)] in enumerator order"""
    m = n - 6
    return dict(
        grav=[("tau", 0, F64, (m,)), ("wrench", 1, F64, (12,)), ("status", 2, I32, ())],
        link_query=[("pos", 0, F64, (q, 3)), ("rot", 1, F64, (q, 3, 3)), ("vel", 2, F64, (q, 6)), ("jac", 3, F64, (q, 6, n))],
        dynamics=[("A", 0, F64, (n, n)), ("A_inv", 1, F64, (n, n)), ("B", 2, F64, (n,)), ("G", 3, F64, (n,)), ("CMM", 4, F64, (6, n)), ("com", 5, F64, (3,)),
                  ("status", 6, I32, ())],
        contact_space=[("J_C", 0, F64, (12, n)), ("Lambda_c", 1, F64, (12, 12)), ("J_C_INV_T", 2, F64, (12, n)), ("N_C", 3, F64, (n, n)),
                       ("A_inv_N_C", 4, F64, (n, n)), ("W", 5, F64, (m, m)), ("W_inv", 6, F64, (m, m)), ("NwJw", 7, F64, (m, 6)),
                       ("contact_pos", 8, F64, (2, 3)), ("contact_rot", 9, F64, (2, 3, 3)), ("status", 10, I32, ())],
    )


def _rows(family, n, q):
    from libdwbc_amd import _lib

    L = _lib.load()
    rows = []
    while True:
        info = _lib.FieldInfo()
        if not L.dwbc_lean_output_describe(family, len(rows), n, q, C.byref(info)):
            return rows
        rows.append(info)


@pytest.mark.parametrize("dims", DIMS)
def test_describe_reproduces_the_frozen_table(dims):
    want = _expected(*dims)
    dtypes = {0: F64, 1: I32}
    for f, fam in enumerate(FAMILIES):
        rows = _rows(f, *dims)
        assert [r.name.decode() for r in rows] == [w[0] for w in want[fam]], fam
        for r, (name, what, dt, shape) in zip(rows, want[fam]):
            assert (r.id, dtypes[r.dtype], tuple(r.dims[: r.rank])) == (what, dt, shape), (fam, name)
            assert tuple(r.dims[r.rank :]) == (1,) * (3 - r.rank), (fam, name)
            assert r.bytes == int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize, (fam, name)
            assert (r.bindable, r.host_mirror) == (1, 0), (fam, name)


def test_describe_ends_and_needs_its_arguments():
    from libdwbc_amd import _lib

    L = _lib.load()
    info = _lib.FieldInfo()
    for f, fam in enumerate(FAMILIES):
        n_rows = len(_expected(*DIMS[0])[fam])
        assert len(_rows(f, *DIMS[0])) == n_rows
        assert L.dwbc_lean_output_describe(f, n_rows, 39, 1, C.byref(info)) == 0
        assert L.dwbc_lean_output_describe(f, -1, 39, 1, C.byref(info)) == 0
        assert L.dwbc_lean_output_describe(f, 0, 39, 1, None) == 0
    assert L.dwbc_lean_output_describe(-1, 0, 39, 1, C.byref(info)) == 0
    assert L.dwbc_lean_output_describe(len(FAMILIES), 0, 39, 1, C.byref(info)) == 0


def _enum(name):
    txt = open(os.path.join(ROOT, "include", "dwbc_batch.h")).read()
    body = re.search(r"enum %s\s*\{(.*?)\};" % name, txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return {e: int(val) for e, val in re.findall(r"\b(DWBC_[A-Za-z0-9_]+)\s*=\s*(\d+)", body)}


def test_one_row_per_enumerator():
    assert _enum("dwbc_lean_family") == {"DWBC_LEAN_" + fam.upper(): f for f, fam in enumerate(FAMILIES)}
    for f, fam in enumerate(FAMILIES):
        name, prefix = ENUMS[fam]
        enum = _enum(name)
        rows = _rows(f, *DIMS[0])
        assert sorted(enum.values()) == list(range(len(enum))) == [r.id for r in rows], fam
        # the names are the enumerators' own, as Python has always spelt them
        by_id = {v: e for e, v in enum.items()}
        assert [r.name.decode().lower() for r in rows] == [by_id[r.id][len(prefix):].lower() for r in rows], fam


def test_python_keeps_no_copy():
    from libdwbc_amd import batch

    want = _expected(*DIMS[0])
    dicts = dict(grav=batch.GRAV_OUTPUTS, link_query=batch.LINK_QUERY_OUTPUTS, dynamics=batch.DYNAMICS_OUTPUTS, contact_space=batch.CONTACT_SPACE_OUTPUTS)
    for f, fam in enumerate(FAMILIES):
        assert list(dicts[fam].items()) == [(w[0], w[1]) for w in want[fam]], fam
        assert dicts[fam] == {r.name.decode(): r.id for r in _rows(f, *DIMS[0])}, fam
    src = open(os.path.join(ROOT, "libdwbc_amd", "batch.py")).read()
    for gone in ("_grav_shape", "_link_query_shape", "_dynamics_shape", "_contact_space_shape"):
        assert gone not in src, gone
