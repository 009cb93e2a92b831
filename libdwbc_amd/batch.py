"""Host-side mirror of libdwbc's RobotData call sequence for a batch of B robots (reference include/dwbc.h).

    model = Model.from_urdf(path)                      # RobotData::LoadModelData
    wbc = Batch(model, B, device=0)
    wbc.add_contact(link, point, lx, ly)               # AddContactConstraint
    wbc.add_task(level, mode, link)                    # AddTaskSpace
    wbc.set_torque_limit(lim)                          # SetTorqueLimit
    wbc.set_state(q); wbc.set_contact(flags); wbc.set_fstar(level, f)   # UpdateKinematics / SetContact / SetTaskSpace
    wbc.solve()                                        # CalcContactConstraint .. CalcContactRedistribute, one launch
    tau = wbc.get("tau_total")
    wbc.set_torque_input(tau_policy); wbc.redistribute()   # CalcContactRedistribute(torque_input): any torque, its own lean kernel
    tau_policy + wbc.get("redist_tau")
    wbc.grav_compensation(); wbc.grav_outputs()["tau"]       # CalcGravCompensation on its own; redistribute(add_gravity=True) adds it to the input
    wbc.set_link_query([0, 23], jacobians=True); wbc.update_kinematics()   # UpdateKinematics on its own: link_[i].xpos / rotm / v / w / jac_
    wbc.link_states()["rot"]
    wbc.set_dynamics_outputs(["A", "B", "CMM"]); wbc.update_dynamics()   # the dynamics half of UpdateKinematics: rd_.A_ / A_inv_ / B_ / G_ / CMM_
    wbc.dynamics()["A"]
    wbc.set_contact_space_outputs(["N_C", "A_inv_N_C", "J_C"]); wbc.calc_contact_constraint()   # SetContact + CalcContactConstraint: the contact space
    wbc.contact_space()["N_C"]

All arithmetic happens in libdwbc_hip.so (hand-written HIP, gfx950).  torch is only used, optionally, to own
device buffers and streams (bind_tensor) and for torch.distributed in bench.py.
"""
import ctypes as C

import numpy as np

from . import _lib

CONTACT_6D = 0
TASK_LINK_6D, TASK_LINK_6D_COM_FRAME, TASK_LINK_6D_CUSTOM_FRAME = 0, 1, 2
TASK_LINK_POSITION, TASK_LINK_POSITION_COM_FRAME, TASK_LINK_POSITION_CUSTOM_FRAME = 3, 4, 5
TASK_LINK_ROTATION, TASK_LINK_ROTATION_CUSTOM_FRAME = 6, 7
SOLVE_HQP, SOLVE_INIT, SOLVE_REDUCED = 1, 2, 4
REDIST_ADD_GRAVITY = 8  # a bit of the redistribution entry points' flags


def describe(index, n, n_contacts, fstar_total, max_active):
    """row `index` of the library's field table (libdwbc_amd/csrc/dwbc_fields.h) for these sizes, None past the end"""
    info = _lib.FieldInfo()
    ok = _lib.load().dwbc_field_describe(index, C.byref(_lib.FieldDims(n, n_contacts, fstar_total, max_active)), C.byref(info))
    return info if ok else None


def describe_lean(family, index, n, n_queried):
    """row `index` of a lean launch's outputs (same file) for a model of n dof and a link query of n_queried entries, None past the end"""
    info = _lib.FieldInfo()
    return info if _lib.load().dwbc_lean_output_describe(family, index, n, n_queried, C.byref(info)) else None


# name -> field id of include/dwbc_batch.h, and name -> row of the table: read from the library once
FIELDS, _ROW = {}, {}
while (_r := describe(len(_ROW), 0, 0, 0, 0)) is not None:
    FIELDS[_r.name.decode()], _ROW[_r.name.decode()] = _r.id, len(_ROW)
_DTYPES = (np.float64, np.int32, np.uint8)  # DWBC_ELEM_*
# enum dwbc_lean_family, as the entry points (dwbc_batch_get_<family>, ...) and the keys of bound tensors spell it; per family
# name -> enumerator of its output enum, read from the library once
LEAN_FAMILIES = ("grav", "link_query", "dynamics", "contact_space")
_LEAN = [{} for _ in LEAN_FAMILIES]
for _f, _d in enumerate(_LEAN):
    while (_r := describe_lean(_f, len(_d), 0, 0)) is not None:
        _d[_r.name.decode()] = _r.id
GRAV_OUTPUTS, LINK_QUERY_OUTPUTS, DYNAMICS_OUTPUTS, CONTACT_SPACE_OUTPUTS = _LEAN
_GRAV, _LINK_QUERY, _DYNAMICS, _CONTACT_SPACE = range(4)


def describe_task_space(index, n, t):
    """output `index` of the task-space launch (same file) for a model of n dof and a level of t task dof, None past the end"""
    info = _lib.FieldInfo()
    return info if _lib.load().dwbc_task_space_output_describe(index, n, t, C.byref(info)) else None


# name -> enumerator of enum dwbc_task_space_output: no lean family (every output but the status exists once per task level), read from
# the library once
TASK_SPACE_OUTPUTS = {}
while (_r := describe_task_space(len(TASK_SPACE_OUTPUTS), 0, 0)) is not None:
    TASK_SPACE_OUTPUTS[_r.name.decode()] = _r.id


def describe_task_qp(index, n):
    """output `index` of the single-level task-QP launch (same file) for a model of n dof, None past the end"""
    info = _lib.FieldInfo()
    return info if _lib.load().dwbc_task_qp_output_describe(index, n, C.byref(info)) else None


# name -> enumerator of enum dwbc_task_qp_output (a table of its own, like the task-space launch's), read from the library once; its two
# inputs as enum dwbc_task_qp_input names them
TASK_QP_OUTPUTS = {}
while (_r := describe_task_qp(len(TASK_QP_OUTPUTS), 0)) is not None:
    TASK_QP_OUTPUTS[_r.name.decode()] = _r.id
TASK_QP_INPUTS = {"torque_prev": 0, "null": 1}


class DwbcError(RuntimeError):
    pass


def _check(ok):
    if not ok:
        raise DwbcError(_lib.last_error())


def tree_tag(parents):
    """name tag of a tree-specific kernel pack: FNV-1a over the parent table as little-endian 32-bit words (dwbc_capi.hip: tree_tag)"""
    h = 2166136261
    for p in parents:
        for b in int(max(p, 0)).to_bytes(4, "little"):
            h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return f"{h:08x}"


def build_pack(model_or_ndof, nb=None, quiet=True, tree=False):
    """Compile the cycle kernels for a model size other than TOCABI's (libdwbc_amd/csrc/dwbc_pack.hip -> libdwbc_pack_<N>_<NB>.so next
    to libdwbc_hip.so; about two minutes with hipcc, nothing to do when it is up to date).  dwbc_batch_create loads it by itself.
    tree=True (needs a Model): a pack for exactly this model's kinematic tree (libdwbc_pack_<N>_<NB>_t<tag>.so) -- the tree-sparse
    A^-1 sweep and compile-time round counts the built-in TOCABI kernels have; it is preferred over the generic pack of the size."""
    import os
    import subprocess

    if nb is None:
        n, nb = int(model_or_ndof.ndof), int(model_or_ndof.nb)
    else:
        n, nb = int(model_or_ndof), int(nb)
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    cmd = ["make", "-C", csrc, "pack", f"N={n}", f"NB={nb}"]
    name = f"libdwbc_pack_{n}_{nb}.so"
    if tree:
        parents = [max(int(p), 0) for p in model_or_ndof.arrays()["parent"]]
        tag = tree_tag(parents)
        cmd += ["PARENTS=" + ",".join(str(p) for p in parents), f"TAG={tag}"]
        name = f"libdwbc_pack_{n}_{nb}_t{tag}.so"
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL if quiet else None)
    return os.path.join(os.path.dirname(csrc), name)


class Model:
    def __init__(self, handle):
        self._L = _lib.load()
        self._h = handle
        self.nb = self._L.dwbc_model_num_links(handle)
        self.ndof = self._L.dwbc_model_system_dof(handle)
        self.total_mass = self._L.dwbc_model_total_mass(handle)

    @classmethod
    def from_urdf(cls, path, floating=True):
        L = _lib.load()
        h = L.dwbc_model_create_from_urdf(str(path).encode(), 1 if floating else 0)
        if not h:
            raise DwbcError(_lib.last_error())
        return cls(h)

    @classmethod
    def from_arrays(cls, m):
        L = _lib.load()
        arrs = [np.ascontiguousarray(m["parent"], np.int32)] + [
            np.ascontiguousarray(m[k], np.float64) for k in ("R_T", "p_T", "axis", "mass", "com", "inertia")
        ]
        h = L.dwbc_model_create_from_arrays(int(m["nb"]), *[a.ctypes.data for a in arrs])
        if not h:
            raise DwbcError(_lib.last_error())
        return cls(h)

    def link_id(self, name):
        return self._L.dwbc_model_link_id(self._h, name.encode())

    # ---- init-time model surgery (RobotData::DeleteLink / AddLink / ChangeLinkToFixedJoint / ChangeLinkInertia, src/dwbc.cpp:1764-2382,
    #      2707-2730): each returns a NEW Model; a model of another size runs on its own kernel pack (build_pack)
    def _link(self, link):
        i = self.link_id(link) if isinstance(link, str) else int(link)
        if i < 0:
            raise DwbcError(f"no link named {link}")
        return i

    def _new(self, h):
        if not h:
            raise DwbcError(_lib.last_error())
        return Model(h)

    def delete_link(self, link):
        return self._new(self._L.dwbc_model_delete_link(self._h, self._link(link)))

    def add_link(self, parent, name, joint_type, joint_axis, joint_rotm, joint_trans, mass, com, inertia):
        """joint_type: 0 fixed (joined to the parent link), 1 revolute (a new last link; the parent must be the last link or one of
        its ancestors).  joint_rotm: rotation child -> parent of the joint frame"""
        a = [np.ascontiguousarray(x, np.float64) for x in (joint_axis, joint_rotm, joint_trans, com, inertia)]
        return self._new(self._L.dwbc_model_add_link(self._h, self._link(parent), str(name).encode(), int(joint_type), a[0].ctypes.data, a[1].ctypes.data,
                                                     a[2].ctypes.data, float(mass), a[3].ctypes.data, a[4].ctypes.data))

    def change_link_to_fixed_joint(self, link):
        return self._new(self._L.dwbc_model_change_link_to_fixed_joint(self._h, self._link(link)))

    def change_link_inertia(self, link, com_inertia, com_position, com_mass):
        a = [np.ascontiguousarray(x, np.float64) for x in (com_inertia, com_position)]
        return self._new(self._L.dwbc_model_change_link_inertia(self._h, self._link(link), a[0].ctypes.data, a[1].ctypes.data, float(com_mass)))

    def link_name(self, i):
        return self._L.dwbc_model_link_name(self._h, i).decode()

    def arrays(self):
        nb = self.nb
        out = dict(parent=np.zeros(nb, np.int32), R_T=np.zeros((nb, 3, 3)), p_T=np.zeros((nb, 3)), axis=np.zeros((nb, 3)),
                   mass=np.zeros(nb), com=np.zeros((nb, 3)), inertia=np.zeros((nb, 3, 3)))
        self._L.dwbc_model_get_arrays(self._h, *[out[k].ctypes.data for k in ("parent", "R_T", "p_T", "axis", "mass", "com", "inertia")])
        out["nb"], out["ndof"] = nb, self.ndof
        return out

    def body_table(self):
        """the model as the kernels read it, (nb, 25): per body R_T[9] row-major, p_T[3], axis[3], mass, com[3], Icom xx xy xz yy yz zz"""
        out = np.zeros((self.nb, 25))
        _check(self._L.dwbc_model_body_table(self._h, out.ctypes.data))
        return out

    def instance_model(self, B, mass=None, com=None, inertia=None, p_T=None, R_T=None, axis=None):
        """(B, nb, 25): one body table per instance for Batch.set_instance_model, in the packing of body_table().  mass (B, nb), com
        (B, nb, 3), inertia (B, nb, 3, 3) about the COM (the upper triangle is read), p_T (B, nb, 3), R_T (B, nb, 3, 3), axis (B, nb, 3);
        a field left at None is the model's own."""
        B, nb = int(B), self.nb
        rec = np.broadcast_to(self.body_table(), (B, nb, 25)).copy()

        def put(x, shape, cols):
            if x is None:
                return
            x = np.asarray(x, np.float64)
            assert x.shape == (B, nb) + shape, x.shape
            rec[:, :, cols] = x.reshape(B, nb, -1)

        put(R_T, (3, 3), slice(0, 9))
        put(p_T, (3,), slice(9, 12))
        put(axis, (3,), slice(12, 15))
        put(mass, (), slice(15, 16))
        put(com, (3,), slice(16, 19))
        if inertia is not None:
            I = np.asarray(inertia, np.float64)
            assert I.shape == (B, nb, 3, 3), I.shape
            rec[:, :, 19:25] = I.reshape(B, nb, 9)[:, :, [0, 1, 2, 4, 5, 8]]
        return rec

    def __del__(self):
        try:
            if self._h:
                self._L.dwbc_model_destroy(self._h)
                self._h = None
        except Exception:
            pass


class Batch:
    def __init__(self, model, B, device=0, dtype="f64"):
        self._L = _lib.load()
        self.model = model
        self.B = int(B)
        self.n = model.ndof
        self.m = model.ndof - 6
        self._h = self._L.dwbc_batch_create(model._h, self.B, int(device), {"f64": 0, "f32": 1}[dtype])
        if not self._h:
            raise DwbcError(_lib.last_error())
        self.n_contacts = 0
        self._keep = {}
        self._contact_consts = []  # (lx, ly, mu, mu_z) per registered contact and the batch-wide torque limit: what a missing half of
        self._tau_lim = None       # set_instance_params is filled from
        self._link_query = 0  # entries of set_link_query

    # ---- setup (shared by all instances)
    def add_contact(self, link, point, lx, ly, mu=0.2, mu_z=0.2, contact_type=CONTACT_6D):
        p = np.ascontiguousarray(point, np.float64)
        i = self._L.dwbc_batch_add_contact(self._h, int(link), int(contact_type), p.ctypes.data, lx, ly, mu, mu_z)
        if i < 0:
            raise DwbcError(_lib.last_error())
        self.n_contacts = i + 1
        self._contact_consts.append((float(lx), float(ly), float(mu), float(mu_z)))
        self._keep.pop("instance_params", None)  # (the library dropped the record: its stride counts the contacts)
        return i

    def add_task(self, level, mode, link, point=(0.0, 0.0, 0.0)):
        """AddTaskSpace(level, mode, link, point); ``link = model.link_id("COM")`` is the synthetic COM link.  A second 6D link on a level
        makes it 12 dof wide: the batch then runs the general-contact kernel, which takes link and COM levels alike."""
        p = np.ascontiguousarray(point, np.float64)
        _check(self._L.dwbc_batch_add_task(self._h, int(level), int(mode), int(link), p.ctypes.data))
        self._drop_level_tensors()  # (the library dropped the task-space and task-QP requests: their shapes and level follow the levels)

    def set_torque_limit(self, lim):
        if lim is None:
            _check(self._L.dwbc_batch_set_torque_limit(self._h, None))
            self._tau_lim = None
        else:
            t = np.ascontiguousarray(lim, np.float64)
            assert t.shape == (self.m,)
            _check(self._L.dwbc_batch_set_torque_limit(self._h, t.ctypes.data))
            self._tau_lim = t.copy()

    # ---- per-instance torque limits and contact cone constants (domain randomisation: motor strength, friction, usable foot area)
    @property
    def instance_param_stride(self):
        """doubles per instance of the parameter record: m + 4 * n_contacts"""
        return int(self._L.dwbc_batch_instance_param_stride(self._h))

    def set_instance_params(self, tau_lim=None, contact=None):
        """Per-instance torque limits ``tau_lim`` (B, m) and contact constants ``contact`` (B, n_contacts, 4) = lx, ly, mu, mu_z in
        registration order: they replace set_torque_limit's values and add_contact's constants in every QP row of solve() and
        redistribute().  A missing half is filled from the batch-wide values (a missing ``tau_lim`` needs set_torque_limit first); both
        None drops the record.  Every entry must be finite and > 0.  Refused with a record: solve(reduced=True), solve(hqp=False), LQP /
        JACC.  add_contact drops the record."""
        if tau_lim is None and contact is None:
            _check(self._L.dwbc_batch_set_instance_params(self._h, None))
            return
        if self.n_contacts < 1:
            raise DwbcError("instance parameters: add the contacts first")
        rec = np.empty((self.B, self.instance_param_stride))
        if tau_lim is None:
            if self._tau_lim is None:
                raise DwbcError("instance parameters: no tau_lim given and no batch-wide torque limit to fill it from (set_torque_limit)")
            rec[:, : self.m] = self._tau_lim
        else:
            t = np.asarray(tau_lim, np.float64)
            assert t.shape == (self.B, self.m), t.shape
            rec[:, : self.m] = t
        if contact is None:
            rec[:, self.m :] = np.asarray(self._contact_consts, np.float64).reshape(-1)
        else:
            c = np.asarray(contact, np.float64)
            assert c.shape == (self.B, self.n_contacts, 4), c.shape
            rec[:, self.m :] = c.reshape(self.B, -1)
        _check(self._L.dwbc_batch_set_instance_params(self._h, rec.ctypes.data))

    def bind_instance_params(self, tensor):
        """The record as a caller-owned device tensor of B x instance_param_stride float64, read in place by every later launch (no
        transfer, no validation); None unbinds"""
        if tensor is None:
            _check(self._L.dwbc_batch_bind_instance_params(self._h, None))
            self._keep.pop("instance_params", None)
            return
        assert tensor.is_cuda and tensor.is_contiguous()
        assert tensor.numel() * tensor.element_size() == self.B * self.instance_param_stride * 8, tensor.shape
        _check(self._L.dwbc_batch_bind_instance_params(self._h, C.c_void_p(tensor.data_ptr())))
        self._keep["instance_params"] = tensor

    # ---- per-instance link mass, COM, inertia and joint frames (domain randomisation of the robot itself: payloads, link lengths)
    @property
    def instance_model_shape(self):
        """shape of the per-instance model record: (B, nb, 25)"""
        return (self.B, self.model.nb, int(self._L.dwbc_batch_instance_model_stride(self._h)) // self.model.nb)

    def set_instance_model(self, tables):
        """One body table per instance, (B, nb, 25) as Model.instance_model packs it: while the batch has it, instance i of solve() (every
        launch route of the full-model cycle) and of the six lean launches is computed with table i.  Checked per body (finite, mass > 0,
        inertia diagonal > 0, unit axis and orthonormal R_T for bodies >= 1); a refused record leaves the batch as it was.  None drops it.
        fp64 batches on TOCABI's tree only; refused with a record: solve(reduced=True), three active contacts, task levels of more than
        6 dof, LQP / JACC."""
        if tables is None:
            _check(self._L.dwbc_batch_set_instance_model(self._h, None))
            return
        t = np.ascontiguousarray(tables, np.float64)
        if t.shape != self.instance_model_shape:
            raise DwbcError(f"instance model: shape {t.shape}, expected {self.instance_model_shape}")
        _check(self._L.dwbc_batch_set_instance_model(self._h, t.ctypes.data))

    def bind_instance_model(self, tensor):
        """The record as a caller-owned device tensor of (B, nb, 25) float64, read in place by every later launch (no transfer, no
        validation); None unbinds"""
        if tensor is None:
            _check(self._L.dwbc_batch_bind_instance_model(self._h, None))
            self._keep.pop("instance_model", None)
            return
        assert tensor.is_cuda and tensor.is_contiguous()
        if tuple(tensor.shape) != self.instance_model_shape or tensor.element_size() != 8:
            raise DwbcError(f"instance model: tensor of shape {tuple(tensor.shape)}, expected float64 {self.instance_model_shape}")
        _check(self._L.dwbc_batch_bind_instance_model(self._h, C.c_void_p(tensor.data_ptr())))
        self._keep["instance_model"] = tensor

    @property
    def fstar_size(self):
        return self._L.dwbc_batch_fstar_size(self._h)

    def task_dof(self, level):
        return self._L.dwbc_batch_task_dof(self._h, level)

    # ---- per-cycle inputs (host arrays)
    def set_state(self, q, qdot=None, qddot=None):
        q = np.ascontiguousarray(q, np.float64)
        assert q.shape == (self.B, self.n + 1), q.shape
        qd = None
        if qdot is not None:
            qd = np.ascontiguousarray(qdot, np.float64)
            assert qd.shape == (self.B, self.n), qd.shape
        _check(self._L.dwbc_batch_set_state(self._h, q.ctypes.data, qd.ctypes.data if qd is not None else None, None))

    def add_custom_task(self, level, task_dof):
        """AddTaskSpace(heirarchy, TASK_CUSTOM, task_dof) (reference include/dwbc.h:318)"""
        _check(self._L.dwbc_batch_add_custom_task(self._h, int(level), int(task_dof)))
        self._drop_level_tensors()

    def set_custom_task(self, level, fstar, J):
        """SetTaskSpace(heirarchy, f*, J_task) (reference include/dwbc.h:333): fstar (B, t), J (B, t, n)"""
        J = np.ascontiguousarray(J, np.float64)
        t = self.task_dof(level)
        assert J.shape == (self.B, t, self.n), J.shape
        f = None
        if fstar is not None:
            f = np.ascontiguousarray(fstar, np.float64)
            assert f.shape == (self.B, t), f.shape
        _check(self._L.dwbc_batch_set_custom_task(self._h, int(level), f.ctypes.data if f is not None else None, J.ctypes.data))

    def set_task_gain(self, level, link_index, pos_p, pos_d, pos_a, rot_p, rot_d, rot_a=(0, 0, 0)):
        """TaskLink::SetTaskGain (reference include/dwbc_task.h:108)"""
        arrs = [np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float64), (3,))) for a in (pos_p, pos_d, pos_a, rot_p, rot_d, rot_a)]
        _check(self._L.dwbc_batch_set_task_gain(self._h, int(level), int(link_index), *[a.ctypes.data for a in arrs]))

    def set_trajectory(self, level, link_index, traj):
        """per-instance trajectory records (B, 34): SetTrajectoryQuintic + SetTrajectoryRotation; None clears"""
        if traj is None:
            _check(self._L.dwbc_batch_set_trajectory(self._h, int(level), int(link_index), None))
            return
        t = np.ascontiguousarray(traj, np.float64)
        assert t.shape == (self.B, 34), t.shape
        _check(self._L.dwbc_batch_set_trajectory(self._h, int(level), int(link_index), t.ctypes.data))

    def set_control_time(self, t):
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(t, np.float64), (self.B,)))
        _check(self._L.dwbc_batch_set_control_time(self._h, t.ctypes.data))

    def copy_kinematics_to(self, target):
        """RobotData::CopyKinematicsData(target) (reference include/dwbc.h:375)"""
        _check(self._L.dwbc_batch_copy_kinematics(target._h, self._h))
        target._drop_level_tensors()  # (the task levels came with the set-up: the library dropped the target's task-space and task-QP requests)
        target.n_contacts = self.n_contacts
        target._contact_consts = list(self._contact_consts)
        target._tau_lim = None if self._tau_lim is None else self._tau_lim.copy()

    def set_max_active_contacts(self, n):
        """Contacts that may be active at once in one instance: 2 (default, the product kernels) or 3 -- every solve of the batch then
        runs the general-contact kernel (feet + one hand, ...; hqp = true, tasks on links and on the synthetic COM link,
        ``model.link_id("COM")``) and ``get("wrench")`` is (B, 6 n).  Trajectories, TASK_CUSTOM levels, the dump record, fp32 and
        ``solve(reduced=True)`` are refused there.  The reference stacks any number of flagged contacts (src/dwbc.cpp:445-453)."""
        _check(self._L.dwbc_batch_set_max_active_contacts(self._h, int(n)))

    @property
    def max_active_contacts(self):
        return int(self._L.dwbc_batch_max_active_contacts(self._h))

    def set_contact(self, flags):
        f = np.ascontiguousarray(flags, np.uint8)
        assert f.shape == (self.B, self.n_contacts), f.shape
        _check(self._L.dwbc_batch_set_contact(self._h, f.ctypes.data))

    def set_fstar(self, level, fstar):
        f = np.ascontiguousarray(fstar, np.float64)
        assert f.shape == (self.B, self.task_dof(level)), f.shape
        _check(self._L.dwbc_batch_set_fstar(self._h, int(level), f.ctypes.data))

    def set_fstar_all(self, fstar):
        if fstar.flags["C_CONTIGUOUS"] and fstar.dtype == np.float64 and fstar.ctypes.data == (self._L.dwbc_batch_host_ptr(self._h, FIELDS["in_fstar"]) or 0):
            # the mirror itself (host_view("in_fstar")), filled in place: mark every level as new without copying
            off = 0
            for lv in range(64):
                if off >= fstar.shape[1]:
                    break
                _check(self._L.dwbc_batch_set_fstar(self._h, lv, C.c_void_p(fstar.ctypes.data + 8 * off)))
                off += self.task_dof(lv)
            return
        off = 0
        lv = 0
        while off < fstar.shape[1]:
            t = self.task_dof(lv)
            self.set_fstar(lv, fstar[:, off : off + t])
            off += t
            lv += 1

    def host_view(self, field):
        """numpy view of the page-locked host mirror of an input field ("in_q", "in_contact", "in_fstar", "in_torque"): fill it in place and
        pass it to set_state / set_contact / set_fstar_all / set_torque_input -- the host-side copy is skipped, the upload is one
        asynchronous transfer"""
        shape, dt, nbytes = self._layout(field)
        p = self._L.dwbc_batch_host_ptr(self._h, FIELDS[field])
        if not p:
            raise DwbcError(f"{field} has no host mirror yet (add the contacts / tasks first)")
        return np.frombuffer((C.c_uint8 * nbytes).from_address(p), dtype=dt).reshape(shape)

    # ---- zero-copy device plumbing (torch owns the memory / stream)
    def bind_tensor(self, field, tensor):
        assert tensor.is_cuda and tensor.is_contiguous()
        nbytes = self._L.dwbc_batch_field_bytes(self._h, FIELDS[field])
        assert tensor.numel() * tensor.element_size() == nbytes, (field, tensor.shape, nbytes)
        self._keep[field] = tensor
        _check(self._L.dwbc_batch_bind_device(self._h, FIELDS[field], C.c_void_p(tensor.data_ptr())))

    def set_stream(self, stream_handle):
        _check(self._L.dwbc_batch_set_stream(self._h, C.c_void_p(stream_handle)))

    def enable_dump(self, on=True):
        _check(self._L.dwbc_batch_enable_dump(self._h, 1 if on else 0))

    # ---- the cycle
    def solve(self, hqp=True, init=True, reduced=False):
        """reduced=True: the Reduced* call sequence of the reference (include/dwbc.h:411-416) instead of the full model"""
        _check(self._L.dwbc_batch_solve(self._h, (SOLVE_HQP if hqp else 0) | (SOLVE_INIT if init else 0) | (SOLVE_REDUCED if reduced else 0)))

    def sync(self):
        _check(self._L.dwbc_batch_sync(self._h))

    # ---- CalcContactRedistribute(torque_input, hqp, init) + getContactForce(torque) for a caller-supplied torque
    def set_torque_input(self, tau):
        """torque_input (B, m) of the next redistribute(); a tensor bound as "in_torque" is read in place instead"""
        t = np.ascontiguousarray(tau, np.float64)
        assert t.shape == (self.B, self.m), t.shape
        _check(self._L.dwbc_batch_set_torque_input(self._h, t.ctypes.data))

    def redistribute(self, hqp=True, init=True, add_gravity=False):
        """The contact-null-space torque NwJw c that brings the contact wrenches of the supplied torque back inside the ZMP / friction
        rows and the torque limits (reference include/dwbc.h:297, src/dwbc.cpp:1377-1568): get("redist_tau") (B, m), the QP's answer
        get("redist_cf") (B, 6), the wrench before and after the correction get("redist_wrench") (B, 2, 12), get("redist_status").
        One lean kernel on the batch's stream, asynchronous; reads the state, contact flags and torque limit of the batch and leaves
        every output of solve() alone.  init=False is accepted and runs cold; hqp=False is refused.
        add_gravity: the torque input is a command on top of gravity compensation -- torque_grav_ + torque_input is redistributed in
        the same launch (row 0 of "redist_wrench" is its wrench), and grav_outputs() are written as well."""
        _check(self._L.dwbc_batch_redistribute(self._h, (SOLVE_HQP if hqp else 0) | (SOLVE_INIT if init else 0) | (REDIST_ADD_GRAVITY if add_gravity else 0)))

    def time_redistributes(self, steps, add_gravity=False):
        return self._time("redistribute", steps, SOLVE_HQP | SOLVE_INIT | (REDIST_ADD_GRAVITY if add_gravity else 0))

    def redistribute_kernel_name(self):
        return self._kernel_name("redistribute")

    # ---- what the lean launches share: `family` indexes LEAN_FAMILIES
    def _kernel_name(self, which):
        name = getattr(self._L, f"dwbc_batch_{which}_kernel_name")(self._h).decode()
        if not name:
            raise DwbcError(_lib.last_error())
        return name

    def _time(self, which, steps, *flags):
        """milliseconds of `steps` back-to-back launches behind one warm launch (dwbc_batch_time_<which>)"""
        ms = C.c_float(0)
        _check(getattr(self._L, f"dwbc_batch_time_{which}")(self._h, *flags, int(steps), C.byref(ms)))
        return ms.value

    def _lean_outputs(self, family):
        """name -> (B, ...) array of every output the family's request holds, shaped and typed by the library's table.  With no request
        the first output is asked for all the same: its refusal says what is missing."""
        fam = LEAN_FAMILIES[family]
        nbytes = {name: getattr(self._L, f"dwbc_batch_{fam}_bytes")(self._h, what) for name, what in _LEAN[family].items()}
        out = {}
        for name, what in _LEAN[family].items():
            if nbytes[name] == 0 and any(nbytes.values()):
                continue
            r = describe_lean(family, what, self.n, self._link_query)
            a = np.zeros((self.B,) + tuple(r.dims[: r.rank]), _DTYPES[r.dtype])
            _check(getattr(self._L, f"dwbc_batch_get_{fam}")(self._h, what, a.ctypes.data, a.nbytes))
            out[name] = a
        return out

    def _lean_bind(self, family, name, tensor):
        fam, what = LEAN_FAMILIES[family], _LEAN[family][name]
        bind = getattr(self._L, f"dwbc_batch_bind_{fam}")
        if tensor is None:
            _check(bind(self._h, what, None))
            self._keep.pop(f"{fam}_{name}", None)
            return
        assert tensor.is_cuda and tensor.is_contiguous()
        nbytes = getattr(self._L, f"dwbc_batch_{fam}_bytes")(self._h, what)
        assert nbytes == 0 or tensor.numel() * tensor.element_size() == nbytes, (name, tensor.shape, nbytes)
        _check(bind(self._h, what, C.c_void_p(tensor.data_ptr())))
        self._keep[f"{fam}_{name}"] = tensor

    def _lean_set_outputs(self, family, names):
        fam = LEAN_FAMILIES[family]
        mask = 0
        for k in names:
            mask |= 1 << _LEAN[family][k]
        _check(getattr(self._L, f"dwbc_batch_set_{fam}_outputs")(self._h, mask))
        for k in _LEAN[family]:
            self._keep.pop(f"{fam}_{k}", None)

    # ---- CalcGravCompensation on its own (reference include/dwbc.h:246-247, src/wbd.cpp:186-192)
    def grav_compensation(self):
        """torque_grav_ and getContactForce(torque_grav_) of the state and contact flags, in one lean kernel on the batch's stream,
        asynchronous: no task space, no torque input, no QP.  Leaves every output of solve(), redistribute() and update_kinematics() as it
        is.  No contact: zeros, status 1; more than two flags or a failed contact stage: zeros, status 0.  fp64, two contacts at most."""
        _check(self._L.dwbc_batch_grav_compensation(self._h))

    def grav_outputs(self):
        """dict of ``tau`` (B, m), ``wrench`` (B, 12) zero padded and ``status`` (B,) int32 of the last grav_compensation() or
        redistribute(add_gravity=True); synchronises the stream"""
        return self._lean_outputs(_GRAV)

    def bind_grav(self, name, tensor):
        """output ``name`` ("tau", "wrench": float64; "status": int32) into a caller-owned device tensor, written in place by every later
        launch; None: back to a buffer of the batch's own"""
        self._lean_bind(_GRAV, name, tensor)

    def grav_kernel_name(self):
        return self._kernel_name("grav")

    def time_grav(self, steps):
        return self._time("grav", steps)

    # ---- UpdateKinematics on its own: poses, velocities and Jacobians of queried links before any f* is set
    def set_link_query(self, links, points=None, jacobians=False):
        """The links update_kinematics() reports: up to 16 entries ``links`` with ``points`` (L, 3) in the links' frames (None: the
        origins); ``model.link_id("COM")`` is the synthetic COM link, which takes no point.  ``jacobians``: also the 6 x n point Jacobians,
        rows [linear; angular] -- what set_custom_task takes.  An empty list drops the query.  A new query has new output buffers: bind
        tensors after it."""
        l = np.ascontiguousarray(links, np.int32).reshape(-1)
        p = None
        if points is not None:
            p = np.ascontiguousarray(points, np.float64)
            assert p.shape == (len(l), 3), p.shape
        _check(self._L.dwbc_batch_set_link_query(self._h, len(l), l.ctypes.data, p.ctypes.data if p is not None else None, 1 if jacobians else 0))
        for k in LINK_QUERY_OUTPUTS:
            self._keep.pop("link_query_" + k, None)
        self._link_query = len(l)

    def update_kinematics(self):
        """One lean kernel on the batch's stream, asynchronous: forward kinematics of the state (and of qdot, if set_state got one; zero
        velocities otherwise) for the queried links.  Reads the state alone and leaves every output of solve() and redistribute() as it
        is; the three may be called in any order."""
        _check(self._L.dwbc_batch_update_kinematics(self._h))

    def link_states(self):
        """dict of ``pos`` (B, L, 3), ``rot`` (B, L, 3, 3) row-major, ``vel`` (B, L, 6) = [v of the point; w] and, if the query asked for
        them, ``jac`` (B, L, 6, n) of the last update_kinematics(); synchronises the stream"""
        return self._lean_outputs(_LINK_QUERY)

    def bind_link_query(self, name, tensor):
        """output ``name`` ("pos", "rot", "vel", "jac") of update_kinematics() into a caller-owned device tensor of float64, written in
        place by every later launch; None: back to a buffer of the batch's own"""
        self._lean_bind(_LINK_QUERY, name, tensor)

    def link_query_kernel_name(self):
        return self._kernel_name("link_query")

    # ---- the dynamics half of UpdateKinematics on its own: rd_.A_, A_inv_, B_, G_, CMM_, com_pos (reference src/dwbc.cpp:279-371)
    def set_dynamics_outputs(self, names):
        """The outputs update_dynamics() writes: any of "A" (n, n), "A_inv" (n, n), "B" (n), "G" (n), "CMM" (6, n), "com" (3); "status" is
        always written.  What is not asked for is not computed: no "A_inv", no sweep; no "B", no RNEA; neither "CMM" nor "com", no centroidal
        block.  An empty list drops the request and its buffers.  A new request has new output buffers: bind tensors after it."""
        self._lean_set_outputs(_DYNAMICS, names)

    def update_dynamics(self):
        """One lean kernel on the batch's stream, asynchronous: kinematics, CRBA and what the request asks for, from the state (and qdot, if
        set_state got one; "B" is "G" to the bit otherwise).  Needs no contact and no task space, and leaves every output of solve(),
        redistribute(), grav_compensation() and update_kinematics() as it is; the five may be called in any order."""
        _check(self._L.dwbc_batch_update_dynamics(self._h))

    def dynamics(self):
        """dict of the asked-for outputs and ``status`` (B,) int32 (0: "A_inv" was asked for and the sweep met a bad pivot; that instance's
        outputs are zero) of the last update_dynamics(); synchronises the stream"""
        return self._lean_outputs(_DYNAMICS)

    def bind_dynamics(self, name, tensor):
        """asked-for output ``name`` of update_dynamics() into a caller-owned device tensor (float64; "status": int32), written in place by
        every later launch; None: back to a buffer of the batch's own"""
        self._lean_bind(_DYNAMICS, name, tensor)

    def dynamics_kernel_name(self):
        return self._kernel_name("dynamics")

    def time_dynamics(self, steps):
        return self._time("dynamics", steps)

    # ---- SetContact + CalcContactConstraint on their own: the contact-space members of RobotData (reference src/dwbc.cpp:433-478, src/wbd.cpp:108-143)
    def set_contact_space_outputs(self, names):
        """The outputs calc_contact_constraint() writes: any of "J_C" (12, n), "Lambda_c" (12, 12), "J_C_INV_T" (12, n), "N_C" (n, n),
        "A_inv_N_C" (n, n), "W" (m, m), "W_inv" (m, m), "NwJw" (m, 6), "contact_pos" (2, 3), "contact_rot" (2, 3, 3); "status" is always
        written.  The shapes are fixed whatever the support: zero beyond the active contact dof.  What is not asked for is not computed: only
        "J_C" / the frames, no A^-1 sweep; no "W_inv", no 33-pivot sweep; no "N_C", no n x n product.  An empty list drops the request and its
        buffers.  A new request has new output buffers: bind tensors after it."""
        self._lean_set_outputs(_CONTACT_SPACE, names)

    def calc_contact_constraint(self):
        """One lean kernel on the batch's stream, asynchronous: kinematics, CRBA, the contact stage and what the request asks for, from the
        state and the contact flags (set_contact, or flags bound on the device).  Needs no task space, and leaves every output of solve(),
        redistribute(), grav_compensation(), update_kinematics() and update_dynamics() as it is; the six may be called in any order."""
        _check(self._L.dwbc_batch_calc_contact_constraint(self._h))

    def contact_space(self):
        """dict of the asked-for outputs and ``status`` (B,) int32 (the return value of CalcContactConstraint; 0: that instance's outputs
        are zero) of the last calc_contact_constraint(); synchronises the stream"""
        return self._lean_outputs(_CONTACT_SPACE)

    def bind_contact_space(self, name, tensor):
        """asked-for output ``name`` of calc_contact_constraint() into a caller-owned device tensor (float64; "status": int32), written in
        place by every later launch; None: back to a buffer of the batch's own"""
        self._lean_bind(_CONTACT_SPACE, name, tensor)

    def contact_space_kernel_name(self):
        return self._kernel_name("contact_space")

    def time_contact_space(self, steps):
        return self._time("contact_space", steps)

    # ---- SetTaskSpace + CalcTaskSpace on their own: ts_[i].J_task_ / Lambda_task_ / J_kt_ / Null_task_ (reference src/dwbc.cpp:795-816, src/wbd.cpp:207-261)
    def set_task_space_outputs(self, names):
        """The outputs calc_task_space() writes per task level of t dof: any of "J_task" (t, n), "Lambda_task" (t, t), "J_kt" (m, t) and
        "Null_task" (m, m; every level but the last); "status" is always written.  What is not asked for is not computed: only "J_task",
        nothing behind the kinematics; neither "J_kt" nor "Null_task", nothing behind Lambda_task; no "Null_task", no projector.  An empty
        list drops the request and its buffers, and so does every change of the task levels.  A new request has new output buffers: bind
        tensors after it."""
        mask = 0
        for k in names:
            mask |= 1 << TASK_SPACE_OUTPUTS[k]
        _check(self._L.dwbc_batch_set_task_space_outputs(self._h, mask))
        self._drop_task_space_tensors()

    def _drop_task_space_tensors(self):
        for k in [k for k in self._keep if k.startswith("task_space_")]:
            del self._keep[k]

    def _drop_level_tensors(self):
        """the task levels changed: the library dropped the task-space request, and the task-QP request with its inputs (a new
        task-space request alone leaves the task-QP launch's bound tensors in use: they stay held)"""
        self._drop_task_space_tensors()
        for k in [k for k in self._keep if k.startswith("task_qp_")]:
            del self._keep[k]

    def calc_task_space(self):
        """One lean kernel on the batch's stream, asynchronous: kinematics, CRBA, the contact stage and, per task level, what the request
        asks for, from the state and the contact flags.  Reads no f*, and leaves every output of solve() and of the other lean launches as
        it is; they may be called in any order."""
        _check(self._L.dwbc_batch_calc_task_space(self._h))

    def _task_space_get(self, level, name):
        what = TASK_SPACE_OUTPUTS[name]
        r = describe_task_space(what, self.n, self.task_dof(level) if name != "status" else 0)
        a = np.zeros((self.B,) + tuple(r.dims[: r.rank]), _DTYPES[r.dtype])
        _check(self._L.dwbc_batch_get_task_space(self._h, int(level), what, a.ctypes.data, a.nbytes))
        return a

    def task_space(self, level=None):
        """The asked-for outputs of the last calc_task_space(); synchronises the stream.  ``level`` given: a dict name -> (B, ...) array of
        that level.  None: ``(levels, status)``, a list of such dicts, one per level, and the status (B,) int32 (0: that instance's
        outputs are zero)."""
        status = self._task_space_get(0, "status")  # (refused without a request or before the first launch: nothing else is asked then)

        def one(l):
            return {k: self._task_space_get(l, k) for k, w in TASK_SPACE_OUTPUTS.items()
                    if k != "status" and self._L.dwbc_batch_task_space_bytes(self._h, l, w)}

        if level is not None:
            return one(int(level))
        n_levels = 0
        while self.task_dof(n_levels) > 0:  # (0 past the last level)
            n_levels += 1
        return [one(l) for l in range(n_levels)], status

    def bind_task_space(self, level, name, tensor):
        """asked-for output ``name`` of ``level`` into a caller-owned device tensor (float64; "status": int32), written in place by every
        later launch; None: back to a buffer of the batch's own"""
        what, key = TASK_SPACE_OUTPUTS[name], f"task_space_{level}_{name}"
        if tensor is None:
            _check(self._L.dwbc_batch_bind_task_space(self._h, int(level), what, None))
            self._keep.pop(key, None)
            return
        assert tensor.is_cuda and tensor.is_contiguous()
        nbytes = self._L.dwbc_batch_task_space_bytes(self._h, int(level), what)
        assert nbytes == 0 or tensor.numel() * tensor.element_size() == nbytes, (name, tensor.shape, nbytes)
        _check(self._L.dwbc_batch_bind_task_space(self._h, int(level), what, C.c_void_p(tensor.data_ptr())))
        self._keep[key] = tensor

    def task_space_kernel_name(self):
        return self._kernel_name("task_space")

    def time_task_space(self, steps):
        return self._time("task_space", steps)

    # ---- CalcSingleTaskTorqueWithQP for one task level on its own: the constrained level solve (reference include/dwbc.h:354, src/dwbc.cpp:941-1127)
    def set_task_qp(self, level, names=None):
        """The task level calc_single_task_torque_qp() solves and the outputs it writes: any of "f_star_qp" (6), "contact_qp" (6),
        "torque_h" (m), "torque_null_h" (m), "torque_contact" (m); "status" is always written; None: all of them.  An empty list drops the
        request and its buffers, and so does every change of the task levels.  A new request has new output buffers: bind tensors after it.
        The inputs stay."""
        mask = 0
        for k in (TASK_QP_OUTPUTS if names is None else names):
            mask |= 1 << TASK_QP_OUTPUTS[k]
        _check(self._L.dwbc_batch_set_task_qp(self._h, int(level), mask))
        for k in TASK_QP_OUTPUTS:
            self._keep.pop(f"task_qp_{k}", None)

    def set_task_qp_inputs(self, torque_prev, null=None):
        """torque_prev (B, m) and task_null_matrix (B, m, m) of the next calc_single_task_torque_qp(), copied into page-locked mirrors and
        uploaded with the launch; null=None: the identity, as the reference passes for level 0.  An input bound to a tensor is refused here."""
        t = np.ascontiguousarray(torque_prev, np.float64)
        assert t.shape == (self.B, self.m), t.shape
        nl = None
        if null is not None:
            nl = np.ascontiguousarray(null, np.float64)
            assert nl.shape == (self.B, self.m, self.m), nl.shape
        _check(self._L.dwbc_batch_set_task_qp_inputs(self._h, t.ctypes.data, nl.ctypes.data if nl is not None else None))
        if null is None:
            self._keep.pop("task_qp_in_null", None)

    def bind_task_qp_input(self, name, tensor):
        """input ``name`` ("torque_prev": (B, m); "null": (B, m, m)) read in place from a caller-owned device tensor of float64 by every later
        launch; None lets go of it (the null matrix: back to the identity)"""
        which, key = TASK_QP_INPUTS[name], f"task_qp_in_{name}"
        if tensor is None:
            _check(self._L.dwbc_batch_bind_task_qp_input(self._h, which, None, 0))
            self._keep.pop(key, None)
            return
        assert tensor.is_cuda and tensor.is_contiguous()
        _check(self._L.dwbc_batch_bind_task_qp_input(self._h, which, C.c_void_p(tensor.data_ptr()), tensor.numel() * tensor.element_size()))
        self._keep[key] = tensor

    def calc_single_task_torque_qp(self):
        """One lean kernel on the batch's stream, asynchronous: one call of the reference method on every instance -- kinematics, CRBA, the
        contact stage, J_kt and Lambda_task of the level, and the QP in [f_star_qp; contact_qp] with the torque-limit rows (if a limit is set)
        and the ZMP / friction rows of the active contacts, started cold.  Reads the state, the contact flags, f* of the level
        (set_fstar / a bound "in_fstar"), the torque limit, the contact constants, the per-instance parameters and the two inputs, and leaves
        every output of solve() and of the other lean launches as it is."""
        _check(self._L.dwbc_batch_calc_single_task_torque_qp(self._h))

    def task_qp(self):
        """dict of the asked-for outputs and ``status`` (B,) int32 (1: the QP solved; 0: that instance's outputs are zero) of the last
        calc_single_task_torque_qp(); synchronises the stream"""
        out = {}
        for name, what in [("status", TASK_QP_OUTPUTS["status"])] + [(k, w) for k, w in TASK_QP_OUTPUTS.items() if k != "status"]:
            if name != "status" and not self._L.dwbc_batch_task_qp_bytes(self._h, what):
                continue  # (the status is asked for all the same: refused without a request or before the first launch)
            r = describe_task_qp(what, self.n)
            a = np.zeros((self.B,) + tuple(r.dims[: r.rank]), _DTYPES[r.dtype])
            _check(self._L.dwbc_batch_get_task_qp(self._h, what, a.ctypes.data, a.nbytes))
            out[name] = a
        return out

    def bind_task_qp(self, name, tensor):
        """asked-for output ``name`` into a caller-owned device tensor (float64; "status": int32), written in place by every later launch;
        None: back to a buffer of the batch's own"""
        what, key = TASK_QP_OUTPUTS[name], f"task_qp_{name}"
        if tensor is None:
            _check(self._L.dwbc_batch_bind_task_qp(self._h, what, None, 0))
            self._keep.pop(key, None)
            return
        assert tensor.is_cuda and tensor.is_contiguous()
        _check(self._L.dwbc_batch_bind_task_qp(self._h, what, C.c_void_p(tensor.data_ptr()), tensor.numel() * tensor.element_size()))
        self._keep[key] = tensor

    def task_qp_kernel_name(self):
        return self._kernel_name("task_qp")

    def time_task_qp(self, steps):
        return self._time("task_qp", steps)

    def time_solves(self, steps, reduced=False):
        return self._time("solves", steps, SOLVE_HQP | SOLVE_INIT | (SOLVE_REDUCED if reduced else 0))

    def launch_info(self):
        t, l = C.c_int(0), C.c_int(0)
        self._L.dwbc_batch_launch_info(self._h, C.byref(t), C.byref(l))
        return t.value, l.value

    def kernel_name(self):
        return self._L.dwbc_batch_kernel_name(self._h).decode()

    def _layout(self, field):
        """(B, ...) shape, element type and bytes of a field of this batch, from the library's table"""
        r = describe(_ROW[field], self.n, self.n_contacts, self.fstar_size, self.max_active_contacts)
        return (self.B,) + tuple(r.dims[: r.rank]), _DTYPES[r.dtype], self.B * r.bytes

    def get(self, field):
        shape, dt, nbytes = self._layout(field)
        out = np.zeros(shape, dtype=dt)
        assert nbytes == out.nbytes == self._L.dwbc_batch_field_bytes(self._h, FIELDS[field]), (field, nbytes, out.nbytes)
        _check(self._L.dwbc_batch_get(self._h, FIELDS[field], out.ctypes.data, out.nbytes))
        return out

    def close(self):
        if self._h:
            self._L.dwbc_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
