"""The C-ABI and the Python layer of the per-instance model record.  not-gpu: the new symbols are exported, declared and bound, and the model
side -- dwbc_model_body_table, Model.instance_model -- packs what the header documents (a batch needs a device: its stride, the validation
rules, one refusal each, and the kept-state guarantee after a refused set are in tests/test_instance_model_gpu.py::test_refusals)."""
import ctypes
import os

import numpy as np
import pytest

from tests import cases
from tests import instance_model_cases as im

NEW = ("dwbc_model_body_table", "dwbc_batch_instance_model_stride", "dwbc_batch_set_instance_model", "dwbc_batch_bind_instance_model")


def test_symbols_resolve_and_are_declared():
    from libdwbc_amd import _lib

    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(cases.ROOT, "include", "dwbc_batch.h")).read()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in header, name
        assert name in bound and bound[name][1] is ctypes.c_int, name
    assert [len(bound[n][2]) for n in NEW] == [2, 1, 2, 2]
    _lib.load()


def test_python_layer_has_the_entry_points():
    import libdwbc_amd as D
    from libdwbc_amd.rl_bridge import RlWBCBridge

    assert isinstance(D.Batch.instance_model_shape, property)
    for f in (D.Model.body_table, D.Model.instance_model, D.Batch.set_instance_model, D.Batch.bind_instance_model, RlWBCBridge.set_instance_model):
        assert callable(f)


def test_body_table_is_the_documented_layout():
    import libdwbc_amd as D

    model = D.Model.from_urdf(cases.URDF)
    t = model.body_table()
    assert t.shape == (34, 25)
    assert (t == im.pack(dict(model.arrays()))).all()
    # the URDF reader and the oracle's model agree on every field to rounding
    assert np.abs(t - im.pack(im.base_arrays())).max() <= 1e-12
    assert abs(t[:, 15].sum() - model.total_mass) <= 1e-9


def test_instance_model_packs_each_field_where_the_table_has_it():
    import libdwbc_amd as D

    model = D.Model.from_arrays(im.base_arrays())
    f = im.fields()
    rec = model.instance_model(im.B, mass=f["mass"], com=f["com"], inertia=f["inertia"], p_T=f["p_T"])
    assert rec.shape == (im.B, 34, 25) and (rec == im.tables()).all()
    # a field left out is the model's own; R_T and the axis land in their columns
    base = model.body_table()
    assert (model.instance_model(3) == base).all()
    only = model.instance_model(im.B, mass=f["mass"])
    assert (only[:, :, 15] == f["mass"]).all() and (np.delete(only, 15, axis=2) == np.delete(base, 15, axis=1)).all()
    R = np.broadcast_to(np.arange(9.0).reshape(3, 3), (2, 34, 3, 3))
    ax = np.broadcast_to(np.array([0.0, 1.0, 0.0]), (2, 34, 3))
    r2 = model.instance_model(2, R_T=R, axis=ax)
    assert (r2[:, :, 0:9] == np.arange(9.0)).all() and (r2[:, :, 12:15] == [0.0, 1.0, 0.0]).all() and (r2[:, :, 9:12] == base[:, 9:12]).all()
    with pytest.raises(AssertionError):
        model.instance_model(2, mass=f["mass"])
