"""not-gpu: the outputs of the task-space launch as the library describes them (dwbc_task_space_output_describe, the table kTaskSpaceRows of
libdwbc_amd/csrc/dwbc_fields.h): enum dwbc_task_space_output has five consecutive enumerators, the Python dict is the library's, the byte
counts of two model sizes are the documented shapes, and the launch is no fifth lean family."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = ["DWBC_TS_J_TASK", "DWBC_TS_LAMBDA_TASK", "DWBC_TS_J_KT", "DWBC_TS_NULL_TASK", "DWBC_TS_STATUS"]


def _enum():
    txt = open(os.path.join(ROOT, "include", "dwbc_batch.h")).read()
    body = re.search(r"enum dwbc_task_space_output\s*\{(.*?)\};", txt, flags=re.S).group(1)
    return {e: int(v) for e, v in re.findall(r"\b(DWBC_[A-Za-z0-9_]+)\s*=\s*(\d+)", body)}


def _rows(n, t):
    from libdwbc_amd import batch

    out = []
    while (r := batch.describe_task_space(len(out), n, t)) is not None:
        out.append(r)
    return out


def test_enum_has_five_consecutive_enumerators():
    enum = _enum()
    assert list(enum) == WANT and list(enum.values()) == list(range(5))


def test_python_dict_is_the_librarys():
    from libdwbc_amd import batch

    rows = _rows(39, 6)
    enum = _enum()
    assert batch.TASK_SPACE_OUTPUTS == {r.name.decode(): r.id for r in rows}
    assert list(batch.TASK_SPACE_OUTPUTS.values()) == list(range(5))
    # the names are the enumerators' own
    by_id = {v: e for e, v in enum.items()}
    assert [r.name.decode().lower() for r in rows] == [by_id[r.id][len("DWBC_TS_"):].lower() for r in rows]
    assert all(r.bindable and not r.host_mirror for r in rows)
    assert batch.describe_task_space(5, 39, 6) is None and batch.describe_task_space(-1, 39, 6) is None


@pytest.mark.parametrize("n,t", [(39, 6), (39, 3), (37, 6), (37, 3)])
def test_bytes_are_the_documented_shapes(n, t):
    m = n - 6
    want = {"J_task": (t, n), "Lambda_task": (t, t), "J_kt": (m, t), "Null_task": (m, m), "status": ()}
    for r in _rows(n, t):
        shape = tuple(r.dims[: r.rank])
        assert shape == want[r.name.decode()], r.name
        cnt = 1
        for d in shape:
            cnt *= d
        assert r.bytes == cnt * (4 if r.name == b"status" else 8) and r.dtype == (1 if r.name == b"status" else 0)


def test_it_is_no_fifth_lean_family():
    from libdwbc_amd import _lib, batch

    info = _lib.FieldInfo()
    assert _lib.load().dwbc_lean_output_describe(4, 0, 39, 0, C.byref(info)) == 0
    assert len(batch.LEAN_FAMILIES) == 4 and "Null_task" not in batch.FIELDS  # (no new field either)
