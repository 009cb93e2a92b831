"""The C-ABI of the per-instance parameter record: the three entry points are exported and bound (not-gpu), and a kernel pack that
does not carry the library's ABI tag is still refused by the loader (gpu: dwbc_batch_create asks for a device before it looks for a
pack).  BatchIO grew by one pointer with this feature; kernel_abi_tag() folds sizeof(BatchIO) and the source hash in, so packs built
before it carry another tag -- the stale pack here is a stand-in with a tag of its own."""
import ctypes
import os
import subprocess

import pytest

from tests import cases

NEW = ("dwbc_batch_instance_param_stride", "dwbc_batch_set_instance_params", "dwbc_batch_bind_instance_params")


def test_symbols_resolve_and_are_declared():
    from libdwbc_amd import _lib

    L = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(cases.ROOT, "include", "dwbc_batch.h")).read()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    for name in NEW:
        assert hasattr(L, name), name
        assert name + "(" in header, name
        assert name in bound, name
    assert bound[NEW[0]][1] is ctypes.c_int and len(bound[NEW[0]][2]) == 1
    assert len(bound[NEW[1]][2]) == 2 and len(bound[NEW[2]][2]) == 2
    _lib.load()


def test_python_layer_has_the_entry_points():
    import libdwbc_amd as D

    assert isinstance(D.Batch.instance_param_stride, property)
    assert callable(D.Batch.set_instance_params) and callable(D.Batch.bind_instance_params)


@pytest.mark.gpu
def test_stale_pack_is_refused_by_its_tag(tmp_path, monkeypatch):
    """a 37-dof tree no test loads a pack for (both outer wrist joints fixed): with a stand-in pack of that tree's name that reports
    another ABI tag in $DWBC_PACK_DIR the batch is refused; without it the generic pack of the size serves the model"""
    import libdwbc_amd as D
    from libdwbc_amd.batch import tree_tag

    md = D.Model.from_urdf(cases.variant_urdf(tmp_path / "fixed_wrists.urdf", ["L_Wrist2_Joint", "R_Wrist2_Joint"]))
    assert (md.ndof, md.nb) == (37, 32)
    cases.ensure_pack(md)  # the generic pack of the size
    tag = tree_tag([max(int(p), 0) for p in md.arrays()["parent"]])
    stale_dir, empty_dir = tmp_path / "stale", tmp_path / "empty"
    stale_dir.mkdir()
    empty_dir.mkdir()
    src = tmp_path / "stale_pack.c"
    src.write_text("static int rows;\nconst void *dwbc_pack_table(int *count, unsigned *abi_tag) { *count = 0; *abi_tag = 0x5a5a0001u; return &rows; }\n")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(stale_dir / f"libdwbc_pack_37_32_t{tag}.so"), str(src)])
    monkeypatch.setenv("DWBC_PACK_DIR", str(stale_dir))
    with pytest.raises(D.DwbcError, match="was built from another version of the kernels"):
        D.Batch(md, 4, device=0)
    monkeypatch.setenv("DWBC_PACK_DIR", str(empty_dir))
    wbc = D.Batch(md, 4, device=0)
    wbc.add_task(0, D.TASK_LINK_6D, 0)
    assert "<37, 32," in wbc.kernel_name()
    assert wbc.instance_param_stride == 31
    wbc.close()
