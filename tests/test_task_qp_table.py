"""not-gpu: the table of the single-level task-QP launch's outputs (libdwbc_amd/csrc/dwbc_fields.h: kTaskQp, read through
dwbc_task_qp_output_describe) against the names, enumerators, element types and shapes written out below as the pin; enum
dwbc_task_qp_output of include/dwbc_batch.h; and the Python layer, which reads the table and keeps no copy.  The table is one of its own:
the four lean families stay four."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import cases

ROOT = cases.ROOT
F64, I32 = np.float64, np.int32
DIMS = [39, 37]  # two sizes, so that m = n - 6 cannot be mistaken for a constant


def _expected(n):
    """[(name, enumerator, element type, per-instance shape)] in enumerator order"""
    m = n - 6
    return [("f_star_qp", 0, F64, (6,)), ("contact_qp", 1, F64, (6,)), ("torque_h", 2, F64, (m,)), ("torque_null_h", 3, F64, (m,)),
            ("torque_contact", 4, F64, (m,)), ("status", 5, I32, ())]


def _rows(n):
    from libdwbc_amd import _lib

    L = _lib.load()
    rows = []
    while True:
        info = _lib.FieldInfo()
        if not L.dwbc_task_qp_output_describe(len(rows), n, C.byref(info)):
            return rows
        rows.append(info)


@pytest.mark.parametrize("n", DIMS)
def test_describe_reproduces_the_frozen_table(n):
    want = _expected(n)
    dtypes = {0: F64, 1: I32}
    rows = _rows(n)
    assert [r.name.decode() for r in rows] == [w[0] for w in want]
    for r, (name, what, dt, shape) in zip(rows, want):
        assert (r.id, dtypes[r.dtype], tuple(r.dims[: r.rank])) == (what, dt, shape), name
        assert tuple(r.dims[r.rank :]) == (1,) * (3 - r.rank), name
        assert r.bytes == int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize, name
        assert (r.bindable, r.host_mirror) == (1, 0), name


def test_describe_ends_and_needs_its_arguments():
    from libdwbc_amd import _lib

    L = _lib.load()
    info = _lib.FieldInfo()
    n_rows = len(_expected(39))
    assert len(_rows(39)) == n_rows == 6
    assert L.dwbc_task_qp_output_describe(n_rows, 39, C.byref(info)) == 0
    assert L.dwbc_task_qp_output_describe(-1, 39, C.byref(info)) == 0
    assert L.dwbc_task_qp_output_describe(0, 39, None) == 0


def _enum(name):
    txt = open(os.path.join(ROOT, "include", "dwbc_batch.h")).read()
    body = re.search(r"enum %s\s*\{(.*?)\};" % name, txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return {e: int(val) for e, val in re.findall(r"\b(DWBC_[A-Za-z0-9_]+)\s*=\s*(\d+)", body)}


def test_one_row_per_enumerator():
    enum = _enum("dwbc_task_qp_output")
    rows = _rows(39)
    assert sorted(enum.values()) == list(range(len(enum))) == [r.id for r in rows]
    by_id = {v: e for e, v in enum.items()}
    assert [r.name.decode().lower() for r in rows] == [by_id[r.id][len("DWBC_TQ_"):].lower() for r in rows]
    assert _enum("dwbc_task_qp_input") == {"DWBC_TQ_IN_TORQUE_PREV": 0, "DWBC_TQ_IN_NULL": 1}
    assert len(_enum("dwbc_lean_family")) == 4  # (no fifth family: the launch has a table of its own)


def test_python_reads_the_table():
    from libdwbc_amd import batch

    assert list(batch.TASK_QP_OUTPUTS.items()) == [(w[0], w[1]) for w in _expected(39)]
    assert batch.TASK_QP_OUTPUTS == {r.name.decode(): r.id for r in _rows(39)}
    assert batch.TASK_QP_INPUTS == {"torque_prev": 0, "null": 1}
    assert len(batch.LEAN_FAMILIES) == 4
