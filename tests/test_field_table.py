"""not-gpu: the field table of the C-ABI (libdwbc_amd/csrc/dwbc_fields.h, read through dwbc_field_describe) against the names, ids, element
types and shapes the Python layer carried by hand before the table existed, written out below as the pin; and the consumers that must
no longer keep a copy of their own."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import cases

ROOT = cases.ROOT
F64, I32, U8 = np.float64, np.int32, np.uint8
# (n, n_contacts, fstar_total, max_active): two sets, so that n / m = n - 6 / n - 12 and the contact capacity cannot be mistaken for each other
DIMS = [(39, 3, 9, 2), (37, 2, 12, 3)]


def _dump_total(n):
    """doubles in one dump record: the parts of DumpLayout::make(n) (dwbc_types.h), summed"""
    m = n - 6
    return (3 * n * n + 2 * 12 * n + 144 + m * m + 2 * m * 6 + n + 12 + 48 * 9 + 48 * 3 + 4 * 6 * n + 4 * 36 + 3 * 4 * m * 6 + 4 * 6 + 4 * 6 + 6 + 5
            + 6 * n + 3 + 9 + 6 * n + n + 2 * 48 * 3 + 2 * 3 + 2 * 9 + 9 + 2 * 24 * 24 + 24 + 2 * 6 * (n - 12))


def _expected(n, n_contacts, fstar_total, max_active):
    """name -> (id, element type, per-instance shape); diag is DG_COUNT = 90 ints in the product build"""
    m = n - 6
    return dict(
        in_q=(0, F64, (n + 1,)), in_contact=(1, U8, (n_contacts,)), in_fstar=(2, F64, (fstar_total,)), in_torque=(3, F64, (m,)),
        tau=(10, F64, (3, m)), wrench=(11, F64, (6 * max_active,)), status=(12, I32, ()), diag=(13, I32, (90,)),
        redist_tau=(14, F64, (m,)), redist_cf=(15, F64, (6,)), redist_wrench=(16, F64, (2, 12)), redist_status=(17, I32, ()),
        tau_grav=(20, F64, (m,)), tau_task=(21, F64, (m,)), tau_contact=(22, F64, (m,)), tau_total=(23, F64, (m,)),
        A=(30, F64, (n, n)), A_inv=(31, F64, (n, n)), J_C=(32, F64, (12, n)), Lambda_c=(33, F64, (144,)), J_C_INV_T=(34, F64, (12, n)),
        A_inv_N_C=(35, F64, (n, n)), W_inv=(36, F64, (m, m)), NwJw=(37, F64, (m, 6)), G=(38, F64, (n,)), P_C=(39, F64, (12,)),
        link_R=(40, F64, (48, 3, 3)), link_p=(41, F64, (48, 3)), fstar_qp=(42, F64, (4, 6)), contact_qp=(43, F64, (4, 6)),
        cf_redis=(44, F64, (6,)), J_task=(45, F64, (4, 6 * n)), Lambda_task=(46, F64, (4, 36)), J_kt=(47, F64, (4, m * 6)),
        qp_viol=(48, F64, (5,)), dump_raw=(49, F64, (_dump_total(n),)),  # (the one field the Python layer had no name for)
        CMM=(50, F64, (6, n)), com=(51, F64, (3,)), com_inertia=(52, F64, (3, 3)), J_com=(53, F64, (6, n)), B=(54, F64, (n,)),
        link_v=(55, F64, (48, 3)), link_w=(56, F64, (48, 3)), contact_pos=(57, F64, (2, 3)), contact_rot=(58, F64, (2, 3, 3)), zmp=(59, F64, (3, 3)),
        A_R=(60, F64, (24, 24)), A_R_inv=(61, F64, (24, 24)), G_R=(62, F64, (24,)), J_I_nc=(63, F64, (6, n - 12)), J_I_nc_inv_T=(64, F64, (6, n - 12)),
    )


BINDABLE = {"in_q", "in_contact", "in_fstar", "in_torque", "tau", "wrench", "status", "redist_tau", "redist_cf", "redist_wrench", "redist_status"}
MIRRORED = {"in_q", "in_contact", "in_fstar", "in_torque"}


def _rows(dims):
    from libdwbc_amd import _lib

    L = _lib.load()
    rows, d = [], _lib.FieldDims(*dims)
    while True:
        info = _lib.FieldInfo()
        if not L.dwbc_field_describe(len(rows), C.byref(d), C.byref(info)):
            return rows
        rows.append(info)


@pytest.mark.parametrize("dims", DIMS)
def test_describe_reproduces_the_frozen_table(dims):
    want = _expected(*dims)
    rows = _rows(dims)
    assert sorted(r.name.decode() for r in rows) == sorted(want)
    dtypes = {0: F64, 1: I32, 2: U8}
    for r in rows:
        name = r.name.decode()
        fid, dt, shape = want[name]
        assert (r.id, dtypes[r.dtype], tuple(r.dims[: r.rank])) == (fid, dt, shape), name
        assert tuple(r.dims[r.rank :]) == (1,) * (3 - r.rank), name
        assert r.bytes == int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize, name
        assert (bool(r.bindable), bool(r.host_mirror)) == (name in BINDABLE, name in MIRRORED), name


def test_describe_ends_and_needs_its_arguments():
    from libdwbc_amd import _lib

    L = _lib.load()
    d, info = _lib.FieldDims(*DIMS[0]), _lib.FieldInfo()
    n = len(_rows(DIMS[0]))
    assert L.dwbc_field_describe(n, C.byref(d), C.byref(info)) == 0
    assert L.dwbc_field_describe(-1, C.byref(d), C.byref(info)) == 0
    assert L.dwbc_field_describe(0, None, C.byref(info)) == 0 and L.dwbc_field_describe(0, C.byref(d), None) == 0


def _enum_fields():
    txt = open(os.path.join(ROOT, "include", "dwbc_batch.h")).read()
    body = re.search(r"enum dwbc_field\s*\{(.*?)\};", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return {name: int(val) for name, val in re.findall(r"\b(DWBC_[A-Za-z0-9_]+)\s*=\s*(\d+)", body)}


def test_one_row_per_enumerator():
    enum = _enum_fields()
    assert len(enum) >= 50 and len(set(enum.values())) == len(enum)
    ids = [r.id for r in _rows(DIMS[0])]
    assert len(set(ids)) == len(ids)
    assert set(ids) == set(enum.values())
    # the names are the enumerators' own, as Python has always spelt them
    assert {r.name.decode().lower() for r in _rows(DIMS[0])} == {e[len("DWBC_"):].lower() for e in enum}


def test_python_and_facade_keep_no_copy():
    from libdwbc_amd import batch

    assert batch.FIELDS == {r.name.decode(): r.id for r in _rows(DIMS[0])}
    assert batch.FIELDS == {k: v[0] for k, v in _expected(*DIMS[0]).items()}
    src = open(os.path.join(ROOT, "libdwbc_amd", "batch.py")).read()
    assert "lambda" not in src and "_SHAPES" not in src
    assert "* 90" not in open(os.path.join(ROOT, "include", "dwbc_amd.hpp")).read()
    for tool in ("stage_times.py", "stage_times_pair.py", "stage_times_reduced.py", "stage_times_gc.py"):
        assert not re.search(r"_h, 13\b", open(os.path.join(ROOT, "tools", tool)).read()), tool
