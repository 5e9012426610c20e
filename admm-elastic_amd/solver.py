"""Python mirror of the reference's Solver / EnergyTerm / Lame interface for the ADMM hot path.

Same names, argument meaning and error behaviour as the reference classes (file:line cited per
method), sitting on the C ABI in include/admm_hip.h.  All per-iteration work runs in the HIP kernels
of libadmm_hip.so; this file only flattens the scene description, like Solver::initialize does.
"""
import ctypes as C
import os

import numpy as np

from . import capi
from .capi import AdmmHipError, Desc, Stats, check, dptr, f64, i32, iptr, lib

TET_LINEAR, TET_NEOHOOKEAN, TET_STVK, TET_SPLINE_NH, TET_SPLINE_STVK, TET_SPLINE_COROTATED, TET_SPLINE_TABLE, TET_STABLE_NH = 0, 1, 2, 3, 4, 5, 6, 7
LS_LDLT, LS_NCMCGS, LS_UZAWACG = 0, 1, 2


class Lame:
    """src/EnergyTerm.hpp:34-59."""

    def __init__(self, youngs=None, poisson=None, mu=None, lambda_=None):
        if youngs is not None:
            self.mu = youngs / (2.0 * (1.0 + poisson))
            self.lambda_ = youngs * poisson / ((1.0 + poisson) * (1.0 - 2.0 * poisson))
        else:
            self.mu, self.lambda_ = mu, lambda_
        self.limit_min, self.limit_max = -100.0, 100.0

    def bulk_modulus(self):
        return self.lambda_ + (2.0 / 3.0) * self.mu

    @staticmethod
    def rubber():
        return Lame(10000000.0, 0.499)

    @staticmethod
    def soft_rubber():
        return Lame(10000000.0, 0.399)

    @staticmethod
    def very_soft_rubber():
        return Lame(1000000.0, 0.299)


class Settings:
    """Solver::Settings, src/Solver.hpp:39-50 (+ the GPU inner-solver knobs)."""

    def __init__(self, **kw):
        self.timestep_s = 1.0 / 24.0
        self.verbose = 0
        self.admm_iters = 10
        self.gravity = -9.8
        self.linsolver = 0
        self.constraint_w = -1.0
        self.pcg_max_iters = 0
        self.pcg_tol = 0.0
        self.gs_max_iters = 0
        self.gs_tol = -1.0
        self.gs_omega = 0.0
        self.uzawa_max_iters = 0
        self.uzawa_tol = 0.0
        self.soft_modes = 0          # GPU build: end projection of every PCG solve on the k lowest modes of the system matrix (admm_hip_compute_soft_modes)
        self.device = 0
        self.rank = 0
        self.world_size = 1
        self.monitor = 0             # GPU build: ADMM monitor of every step (admm_hip_set_monitor): 0 off, 1 residuals, 2 residuals + objective, 3 = 2 + stationarity
        self.admm_tol = 0.0          # GPU build: early exit of a step's ADMM loop on its residuals (admm_hip_set_admm_stop); 0 = off
        self.admm_min_iters = 1      #            ... but not before this many iterations
        self.anderson = 0            # GPU build: Anderson acceleration of a step's ADMM loop (admm_hip_set_anderson): window 0 (off) .. 8
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError("unknown setting " + k)
            setattr(self, k, v)


class RuntimeData:
    """Solver::RuntimeData, src/Solver.hpp:54-61."""

    def __init__(self):
        self.global_ms = 0.0
        self.local_ms = 0.0
        self.collision_ms = 0.0
        self.local_kernel_ms = 0.0   # tet local-step kernel durations (device clock); local_ms = the phase incl. dispatch gaps
        self.inner_iters = 0
        self.step_ms = 0.0
        self.last_solve_converged = 0
        self.rhs_ms = 0.0
        self.unconverged_solves = 0
        self.pcg_launched_iters = 0
        self.pcg_iters_per_solve = []
        self.admm_iters = 0          # ADMM iterations the step executed (fewer than Settings.admm_iters with Settings.admm_tol > 0)


class Floor:
    """src/PassiveObject.hpp:32-45."""

    def __init__(self, y):
        self.kind, self.params = 0, [float(y), 0.0, 0.0, 0.0]


class Sphere:
    """src/PassiveObject.hpp:48-64."""

    def __init__(self, center, radius):
        self.kind, self.params = 1, [float(center[0]), float(center[1]), float(center[2]), float(radius)]


class Plane:
    """A user-side PassiveCollision (src/Collider.hpp:66-83): the half space n.x < d is solid.  signed distance n.x - d (n normalised),
    contact point x - dx n.  Floor(y) is Plane((0, 1, 0), y)."""

    def __init__(self, normal, d):
        n = f64(normal).ravel()
        l = float(np.linalg.norm(n))
        if not l > 0.0:
            raise AdmmHipError(-1, "Plane: zero normal")
        # unit normal, offset scaled with it -- as the C++ mirror's Plane and the library do: oracle and device see the same plane
        self.kind, self.params = 2, [float(n[0] / l), float(n[1] / l), float(n[2] / l), float(d) / l]


class SampledObstacle:
    """ANY user-defined PassiveCollision on the device: `obj.signed_distance(x) -> (dx, point[3], normal[3])` (the payload a fresh
    Payload would hold after src/Collider.hpp:80-82) is sampled on a dims[0] x dims[1] x dims[2] grid over the box [lo, hi] at
    Solver::initialize (admm_host_sample_obstacle); the kernels interpolate distance and normal trilinearly.  Outside the box the
    object is never hit: make the box cover the region the scene can reach."""

    def __init__(self, obj, lo, hi, dims=(64, 64, 64)):
        self.kind, self.obj = 3, obj
        self.lo, self.hi = f64(lo).ravel().copy(), f64(hi).ravel().copy()
        self.dims = i32(dims).ravel().copy()
        self.params = [0.0, 0.0, 0.0, 0.0]     # params[0] = index of its grid, set by make_desc

    def sample(self):
        n = int(self.dims[0]) * int(self.dims[1]) * int(self.dims[2])
        meta = np.zeros(10); data = np.zeros(4 * n)
        obj = self.obj

        failed = []

        def cb(user, px, pout):
            # a Python exception must not unwind through the C frames, and a sample that was never written must not read as
            # "distance 0, normal 0": NaN makes admm_host_sample_obstacle return ADMM_HIP_ERR_ARG, the exception is re-raised below
            try:
                dx, point, normal = obj.signed_distance(np.array([px[0], px[1], px[2]]))
                vals = [float(dx)] + [float(point[a]) for a in range(3)] + [float(normal[a]) for a in range(3)]
            except Exception as e:
                if not failed:
                    failed.append(e)
                vals = [float("nan")] * 7
            for a in range(7):
                pout[a] = vals[a]
        fn = capi.OBSTACLE_FN(cb)
        rc = lib().admm_host_sample_obstacle(fn, None, dptr(self.lo), dptr(self.hi), iptr(self.dims), dptr(meta), dptr(data))
        if failed:
            raise failed[0]
        check(rc)
        return meta, data


class TetMeshCollision:
    """admm::TetMeshCollision (src/DynamicObject.hpp:31-121): self-collision proxy of one tet mesh.  verts = REST
    vertices of the mesh, tets / faces index them (faces = surface triangles; meshes.surface_faces), v_offset = index
    of the mesh's first vertex in the solver's node vector."""

    def __init__(self, verts, tets, faces, v_offset):
        self.rest = f64(verts).reshape(-1, 3).copy()
        self.tets = i32(tets, (-1, 4)).copy()
        self.faces = i32(faces, (-1, 3)).copy()
        self.vert_offset = int(v_offset)
        if self.faces.shape[0] == 0:
            raise AdmmHipError(-1, "**TetMeshCollision Error: TetMesh needs surface faces")


class Solver:
    """admm::Solver (src/Solver.hpp:32-124) on the MI355X hot path."""

    def __init__(self):
        self.m_x = np.zeros(0)
        self.m_v = np.zeros(0)
        self.m_masses = np.zeros(0)
        self._tets = []   # (idx[n,4], Binv[n,9], weight[n], kind[n], mu[n], la[n], k[n], kappa[n], spline table[n])
        self._user_splines = []   # user-defined xu::Spline objects (TET_SPLINE_TABLE), in order of first use
        self._tris = []   # (idx[n,3], rest[n,4], weight[n], lmin[n], lmax[n])
        self._pins = {}   # vertex -> xyz   (ConstraintSet::pins)
        self._slides = {}  # vertex -> (point, unit normal): slide constraints (README TODO of the reference; include/admm_hip.h: desc.pin_normal)
        self._bends = []   # (idx[n,4], coef[n,4], weight[n], stiffness[n]): bending hinges (desc.bend_*)
        self._obstacles = []
        self._dynamic = []      # TetMeshCollision objects (Collider::dynamic_objs)
        self.surface_inds = []  # Solver::surface_inds (src/Solver.hpp:70): empty = every vertex is tested
        self._ctx = None
        self._settings = Settings()
        self._runtime = RuntimeData()
        self.initialized = False
        self._gs_colors = None
        self._rank, self._world = 0, 1

    def __del__(self):
        self.close()

    def close(self):
        if getattr(self, "_ctx", None):
            lib().admm_hip_destroy(self._ctx)
            self._ctx = None

    # ---- scene construction -------------------------------------------------------------------
    def add_nodes(self, x, m):
        """Solver::add_nodes (src/Solver.hpp:127-141): x, m are [n,3] / [3n] (masses x3). Returns node count."""
        x = f64(x).ravel(); m = f64(m).ravel()
        if x.size != m.size or x.size % 3:
            raise ValueError("add_nodes: x and m must both hold 3 values per node")
        self.m_x = np.concatenate([self.m_x, x])
        self.m_v = np.concatenate([self.m_v, np.zeros_like(x)])
        self.m_masses = np.concatenate([self.m_masses, m])
        return self.m_x.size // 3

    def add_tets(self, verts, inds, lame, kind=TET_LINEAR, vertex_offset=0, spline=None, kappa=0.0):
        """create_tets_from_mesh<IN_SCALAR,TYPE> (src/TetEnergyTerm.hpp:35-51) + the TetEnergyTerm ctor
        (src/TetEnergyTerm.cpp:31-48).  verts are the REST positions the indices refer to; kind selects
        TetEnergyTerm / NeoHookeanTet / StVKTet / SplineTet (TET_SPLINE_*: xu::NeoHookean / StVK / CoRotated with
        their compression term `kappa`, src/XuSpline.hpp:43-45 -- 0 as the reference's SplineTet constructors pass;
        `spline` = a Lame holding the spline's own mu / lambda, default the tet's, as the SplineTet constructors do,
        src/TetEnergyTerm.hpp:192-204).  Raises on an inverted rest tet."""
        inds = i32(inds, (-1, 4))
        Binv, vol = capi.tet_rest(verts, inds)
        k = lame.bulk_modulus()
        n = inds.shape[0]
        w = np.sqrt(k * vol)
        table = 0
        if kind == TET_SPLINE_TABLE:
            # SplineTet(tet, verts, lame, shared_ptr<xu::Spline>) with a USER-DEFINED spline (src/TetEnergyTerm.hpp:197-204): any
            # object with f, g, h, df, dg, dh (src/XuSpline.hpp:34-46); sampled once into a device table
            if spline is None or not all(hasattr(spline, a) for a in ("f", "g", "h", "df", "dg", "dh")):
                raise AdmmHipError(-1, "TET_SPLINE_TABLE needs a spline object with f, g, h, df, dg, dh")
            if not any(spline is sp for sp in self._user_splines):
                self._user_splines.append(spline)
            table = [i for i, sp in enumerate(self._user_splines) if sp is spline][0]
            sp = lame
        else:
            sp = spline if spline is not None else lame
        self._tets.append((inds + vertex_offset, Binv, w, np.full(n, kind, np.int32), np.full(n, sp.mu),
                           np.full(n, sp.lambda_), np.full(n, k), np.full(n, float(kappa) if TET_SPLINE_NH <= kind <= TET_SPLINE_COROTATED else 0.0),
                           np.full(n, table, np.int32)))
        return n

    def add_tris(self, verts, inds, lame, vertex_offset=0):
        """create_tris_from_mesh (src/TriEnergyTerm.hpp:31-46) + TriEnergyTerm ctor (src/TriEnergyTerm.cpp:29-52)."""
        if lame.limit_min > 1.0:
            raise AdmmHipError(-1, "**TriEnergyTerm Error: Strain limit min should be -inf to 1")
        if lame.limit_max < 1.0:
            raise AdmmHipError(-1, "**TriEnergyTerm Error: Strain limit max should be 1 to inf")
        inds = i32(inds, (-1, 3))
        rest, area = capi.tri_rest(verts, inds)
        n = inds.shape[0]
        w = np.sqrt(lame.bulk_modulus() * area)
        self._tris.append((inds + vertex_offset, rest, w, np.full(n, lame.limit_min), np.full(n, lame.limit_max)))
        return n

    def add_bends(self, verts, tris, k_bend, vertex_offset=0):
        """Bending terms for a triangle mesh (README.md:23-28 TODO of the reference; no reference code): one hinge term per interior edge,
        created like create_tris_from_mesh creates the stretch terms (src/TriEnergyTerm.hpp:31-46).  Discrete quadratic bending energy
        (Bergou et al. 2006): E = k_bend * 3 / (A0 + A1) / 2 * |sum_k c_k x_k|^2 with the cotangent stencil c of the REST shape
        (admm_host_bend_hinges); weight = sqrt(stiffness), so that the prox is q / 2 (the idiom of src/TriEnergyTerm.cpp:77-83).
        Returns the number of hinges."""
        idx, coef, area = capi.bend_hinges(verts, tris)
        stiff = float(k_bend) * 3.0 / area
        self._bends.append((idx + vertex_offset, coef, np.sqrt(stiff), stiff))
        return idx.shape[0]

    def set_slide_pins(self, inds, points, normals):
        """Slide constraints (README.md:23-28 TODO of the reference; the counterpart of Solver::set_pins, src/Solver.cpp:113-157, for
        normal-only constraints): vertex inds[i] may move freely in the plane through points[i] with normal normals[i].  Replaces the
        current set of slide constraints; ordinary pins are set_pins' business.  After initialize only constraints created before it may
        be moved / re-oriented (like pins with linsolver 0 / 2, src/Solver.cpp:147-151)."""
        new = {}
        for i, idx in enumerate(inds):
            n = f64(normals[i]).ravel().copy()
            l = float(np.linalg.norm(n))
            if not l > 0.0:
                raise AdmmHipError(-1, "set_slide_pins: zero normal")
            new[int(idx)] = (f64(points[i]).ravel().copy(), n / l)
        left = [k for k in self._slides if k not in new]
        if self.initialized and left:      # a vertex that leaves the set must not keep its normal (it would slide again when pinned later)
            check(lib().admm_hip_set_pin_normals(self._ctx, len(left), iptr(i32(left)), dptr(np.zeros((len(left), 3)))))
        self._slides = new
        if self.initialized:
            self._push_pins()
            v = i32(list(self._slides.keys()))
            nn = f64(np.array([q[1] for q in self._slides.values()]).reshape(-1, 3)) if len(v) else np.zeros((0, 3))
            check(lib().admm_hip_set_pin_normals(self._ctx, len(v), iptr(v), dptr(nn)))

    def _all_pins(self):
        """ordinary pins, then slide pins: (vertex list, points [n,3], normals [n,3] -- zero for ordinary pins)"""
        v = list(self._pins.keys()) + [k for k in self._slides if k not in self._pins]
        pts = [self._pins[k] for k in self._pins] + [self._slides[k][0] for k in self._slides if k not in self._pins]
        nrm = [np.zeros(3) for _ in self._pins] + [self._slides[k][1] for k in self._slides if k not in self._pins]
        return v, (f64(np.array(pts)).reshape(-1, 3) if v else np.zeros((0, 3))), (f64(np.array(nrm)).reshape(-1, 3) if v else np.zeros((0, 3)))

    def _push_pins(self):
        v, p, _ = self._all_pins()
        vi = i32(v)
        check(lib().admm_hip_set_pins(self._ctx, len(vi), iptr(vi), dptr(p)))

    def set_pins(self, inds, points=None):
        """Solver::set_pins (src/Solver.cpp:113-157)."""
        inds = [int(i) for i in inds]
        n = len(inds)
        pin_in_place = points is None or len(points) != n
        if (self.m_x.size == 0 and pin_in_place) or (pin_in_place and points is not None and len(points) > 0):
            raise AdmmHipError(-1, "**Solver::set_pins Error: Bad input.")
        if pin_in_place and self.initialized and self._ctx:
            self.download()     # the reference pins at the CURRENT m_x: after device-resident stepping the host copy is stale
        self._pins = {}
        for i, idx in enumerate(inds):
            self._pins[idx] = self.m_x[3 * idx:3 * idx + 3].copy() if pin_in_place else f64(points[i]).copy()
        if self.initialized:
            self._push_pins()

    def add_obstacle(self, obj):
        """Solver::add_obstacle (src/Solver.cpp:159-161)."""
        self._obstacles.append(obj)

    def set_wind(self, tris, direction):
        """ext_forces.push_back(WindForce(tris)) with WindForce::direction (src/ExplicitForce.hpp:39-46), applied on the device
        at the start of every step.  tris [n,3] node indices; empty = no wind.  After initialize."""
        self._need_ctx()
        t = i32(tris, (-1, 3)) if len(tris) else np.zeros((0, 3), np.int32)
        d = f64(direction).ravel().copy()
        check(lib().admm_hip_set_wind(self._ctx, t.shape[0], iptr(t), dptr(d)))

    def add_dynamic_collider(self, obj):
        """Solver::add_dynamic_collider (src/Solver.cpp:163-165)."""
        self._dynamic.append(obj)

    def detect_dynamic(self, x=None):
        """Collider::detect for the dynamic objects at x (default m_x): list of (vert, dx, face[3], barys[3], normal[3])
        = DynamicCollision::Payload, in candidate order."""
        self._need_ctx()
        x = f64(self.m_x if x is None else x).ravel().copy()
        nv = x.size // 3
        n = C.c_int32(0)
        vert = np.zeros(nv, np.int32); face = np.zeros((nv, 3), np.int32)
        bary = np.zeros((nv, 3)); nrm = np.zeros((nv, 3)); dx = np.zeros(nv)
        check(lib().admm_hip_detect_dynamic(self._ctx, dptr(x), nv, C.byref(n), iptr(vert), iptr(face), dptr(bary), dptr(nrm), dptr(dx)))
        return [(int(vert[i]), dx[i], face[i].copy(), bary[i].copy(), nrm[i].copy()) for i in range(n.value)]

    def set_gs_colors(self, colors):
        self._gs_colors = i32(colors)

    # ---- Solver::initialize (src/Solver.cpp:167-261) ----------------------------------------------
    def flatten(self):
        """Flat arrays of every energy term, in the order tets, tris (pins are appended by the library)."""
        def cat(lst, k, shape, dt):
            return np.concatenate([t[k] for t in lst]).astype(dt) if lst else np.zeros(shape, dt)
        T, R, H = self._tets, self._tris, self._bends
        pv, pp, pn = self._all_pins()
        out = dict(
            bend_idx=cat(H, 0, (0, 4), np.int32), bend_coef=cat(H, 1, (0, 4), np.float64), bend_weight=cat(H, 2, (0,), np.float64),
            bend_stiffness=cat(H, 3, (0,), np.float64), pin_normal=pn,
            tet_idx=cat(T, 0, (0, 4), np.int32), tet_Binv=cat(T, 1, (0, 9), np.float64), tet_weight=cat(T, 2, (0,), np.float64),
            tet_kind=cat(T, 3, (0,), np.int32), tet_mu=cat(T, 4, (0,), np.float64), tet_lambda=cat(T, 5, (0,), np.float64),
            tet_k=cat(T, 6, (0,), np.float64), tet_kappa=cat(T, 7, (0,), np.float64), tet_spline=cat(T, 8, (0,), np.int32),
            tri_idx=cat(R, 0, (0, 3), np.int32), tri_rest=cat(R, 1, (0, 4), np.float64), tri_weight=cat(R, 2, (0,), np.float64),
            tri_limit_min=cat(R, 3, (0,), np.float64), tri_limit_max=cat(R, 4, (0,), np.float64),
            pin_vert=i32(pv), pin_xyz=pp,
        )
        return out

    def make_desc(self, s):
        dof = self.m_x.size
        f = self.flatten()
        self._flat = f  # keep the arrays alive while the descriptor points at them
        d = Desc()
        d.struct_size = C.sizeof(Desc)
        d.device = s.device
        d.n_verts = dof // 3
        self._masses_c = f64(self.m_masses)
        d.masses = dptr(self._masses_c)
        d.dt = s.timestep_s
        d.n_tets = f["tet_idx"].shape[0]
        d.tet_idx, d.tet_Binv, d.tet_weight = iptr(f["tet_idx"]), dptr(f["tet_Binv"]), dptr(f["tet_weight"])
        d.tet_kind, d.tet_mu, d.tet_lambda, d.tet_k = iptr(f["tet_kind"]), dptr(f["tet_mu"]), dptr(f["tet_lambda"]), dptr(f["tet_k"])
        d.tet_kappa = dptr(f["tet_kappa"]) if f["tet_kappa"].any() else None
        if self._user_splines:          # tabulate every user-defined spline (admm_host_tabulate_spline)
            nd = capi.SPLINE_TABLE_DOUBLES
            self._spline_tables = np.zeros((len(self._user_splines), nd))
            for i, sp in enumerate(self._user_splines):
                fns = (sp.f, sp.g, sp.h, sp.df, sp.dg, sp.dh)
                cb = capi.SPLINE_FN(lambda user, which, x, fns=fns: float(fns[which](x)))
                check(lib().admm_host_tabulate_spline(cb, None, float(getattr(sp, "table_min", 0.02)), float(getattr(sp, "table_max", 50.0)),
                                                      dptr(self._spline_tables[i])))
            d.n_spline_tables = len(self._user_splines)
            d.spline_tables = dptr(self._spline_tables)
            d.tet_spline = iptr(f["tet_spline"])
        self._xyz_c = f64(self.m_x).copy()           # smooth coordinates for the coarse space of the on-chip PCG (desc.vert_xyz)
        d.vert_xyz = dptr(self._xyz_c) if self._xyz_c.size == dof else None
        d.n_tris = f["tri_idx"].shape[0]
        d.tri_idx, d.tri_rest, d.tri_weight = iptr(f["tri_idx"]), dptr(f["tri_rest"]), dptr(f["tri_weight"])
        d.tri_limit_min, d.tri_limit_max = dptr(f["tri_limit_min"]), dptr(f["tri_limit_max"])
        d.n_pins = f["pin_vert"].shape[0]
        d.pin_vert, d.pin_xyz, d.pin_active, d.pin_weight = iptr(f["pin_vert"]), dptr(f["pin_xyz"]), None, 0.0
        d.pin_normal = dptr(f["pin_normal"]) if self._slides else None
        d.n_bends = f["bend_idx"].shape[0]
        if d.n_bends:
            d.bend_idx, d.bend_coef = iptr(f["bend_idx"]), dptr(f["bend_coef"])
            d.bend_weight, d.bend_stiffness = dptr(f["bend_weight"]), dptr(f["bend_stiffness"])
        d.linsolver, d.constraint_w = s.linsolver, s.constraint_w
        d.pcg_max_iters, d.pcg_tol = s.pcg_max_iters, s.pcg_tol
        d.gs_max_iters, d.gs_tol, d.gs_omega = s.gs_max_iters, s.gs_tol, s.gs_omega
        d.uzawa_max_iters, d.uzawa_tol = s.uzawa_max_iters, s.uzawa_tol
        metas, datas, nodes = [], [], 0
        for o in self._obstacles:          # user-defined obstacles: sampled now, like Solver::initialize would first call them
            if o.kind == 3:
                meta, data = o.sample()
                meta[9] = nodes; o.params = [float(len(metas)), 0.0, 0.0, 0.0]
                metas.append(meta); datas.append(data); nodes += data.size // 4
        if metas:
            self._grid_meta = np.concatenate(metas); self._grid_data = np.concatenate(datas)
            d.n_obstacle_grids = len(metas); d.obstacle_grid_meta = dptr(self._grid_meta); d.obstacle_grid_data = dptr(self._grid_data)
        self._obst_kind = i32([o.kind for o in self._obstacles])
        self._obst_par = f64([o.params for o in self._obstacles]).reshape(-1, 4) if self._obstacles else np.zeros((0, 4))
        d.n_obstacles = len(self._obstacles)
        d.obstacle_kind, d.obstacle_params = iptr(self._obst_kind), dptr(self._obst_par)
        d.gs_colors = iptr(self._gs_colors) if self._gs_colors is not None else None
        d.rank, d.world_size = s.rank, s.world_size
        return d

    def host_matrix(self, settings=None):
        """Ahat for this scene from the host-only assembly path (no GPU): (rowptr, col, val)."""
        d = self.make_desc(settings if settings is not None else self._settings)
        nnz = C.c_int32(0)
        check(lib().admm_host_assemble_matrix(C.byref(d), None, None, None, C.byref(nnz)))
        nv = self.m_x.size // 3
        rp = np.zeros(nv + 1, np.int32); ci = np.zeros(nnz.value, np.int32); va = np.zeros(nnz.value)
        check(lib().admm_host_assemble_matrix(C.byref(d), iptr(rp), iptr(ci), dptr(va), C.byref(nnz)))
        return rp, ci, va

    def host_oc_plan(self, n_blocks, slices_per_block, lds_bytes=159744, settings=None, coarse=True):
        """The plan the library makes for the on-chip PCG of this scene (admm_host_oc_plan, no GPU): dict(row_vertex,
        row_aggregate, coarse_inv, stats)."""
        d = self.make_desc(settings if settings is not None else self._settings)
        n = 64 * n_blocks * slices_per_block
        rv = np.zeros(n, np.int32); ra = np.zeros(n, np.int32)
        nc = 4 * n_blocks
        ci = np.zeros((nc, nc)) if coarse else None
        st = (C.c_int64 * 11)()
        wt = np.zeros((n, 4), np.float32)
        check(lib().admm_host_oc_plan(C.byref(d), n_blocks, slices_per_block, lds_bytes, iptr(rv), iptr(ra), dptr(ci) if coarse else None, st,
                                      wt.ctypes.data_as(C.POINTER(C.c_float))))
        keys = ("nnz", "stored", "on_chip", "block_local", "max_neighbour_blocks", "coarse_unknowns", "max_halo", "lds_cols")
        stats = dict(zip(keys, list(st)[:8]))
        stats.update(lambda_bb=st[8] * 1e-9, bank_load_by_index=st[9] * 1e-6, bank_load_placed=st[10] * 1e-6)
        return dict(row_vertex=rv, row_aggregate=ra, coarse_inv=ci, stats=stats, row_weights=wt)

    def host_oc_plan_halo(self, n_blocks, slices_per_block, lds_bytes=159744, settings=None):
        """The halo lists of the same plan (admm_host_oc_plan_halo, no GPU): dict(halo_ptr [n_blocks + 1], halo_src, halo_vert) -- the
        internal row of every halo entry and its vertex."""
        d = self.make_desc(settings if settings is not None else self._settings)
        hp = np.zeros(n_blocks + 1, np.int32)
        check(lib().admm_host_oc_plan_halo(C.byref(d), n_blocks, slices_per_block, lds_bytes, iptr(hp), None, None))
        hs = np.zeros(max(int(hp[-1]), 1), np.int32); hv = np.zeros(max(int(hp[-1]), 1), np.int32)
        check(lib().admm_host_oc_plan_halo(C.byref(d), n_blocks, slices_per_block, lds_bytes, iptr(hp), iptr(hs), iptr(hv)))
        return dict(halo_ptr=hp, halo_src=hs[:int(hp[-1])], halo_vert=hv[:int(hp[-1])])

    def host_big_plan(self, max_aggregates=0, settings=None):
        """The plan of the launch-path two-level PCG of this scene (admm_host_big_plan, no GPU): dict(G, ra, rows, nc, ncp, slices, row_vertex,
        row_weights [rows, 4], coarse_inv [nc, nc])."""
        d = self.make_desc(settings if settings is not None else self._settings)
        st = np.zeros(6, np.int32)
        check(lib().admm_host_big_plan(C.byref(d), int(max_aggregates), iptr(st), None, None, None))
        rows, nc = int(st[2]), int(st[3])
        rv = np.zeros(rows, np.int32); wt = np.zeros((rows, 4)); ci = np.zeros((nc, nc), np.float32)
        check(lib().admm_host_big_plan(C.byref(d), int(max_aggregates), iptr(st), iptr(rv), dptr(wt), ci.ctypes.data_as(C.POINTER(C.c_float))))
        return dict(G=int(st[0]), ra=int(st[1]), rows=rows, nc=nc, ncp=int(st[4]), slices=int(st[5]), row_vertex=rv, row_weights=wt, coarse_inv=ci)

    def initialize(self, settings=None):
        s = settings if settings is not None else Settings()
        self._settings = s
        dof = self.m_x.size
        if s.timestep_s <= 0.0:
            s.timestep_s = 1.0 / 24.0
        if not (self.m_masses.size == dof and dof >= 3):
            return False  # "Problem with node data!" (Solver.cpp:180-183)
        self.m_v = np.zeros(dof)
        self.close()
        d = self.make_desc(s)
        ctx = C.c_void_p()
        check(lib().admm_hip_create(C.byref(d), C.byref(ctx)))
        self._ctx = ctx
        if len(self.surface_inds):
            si = i32(self.surface_inds)
            check(lib().admm_hip_set_surface_inds(ctx, len(si), iptr(si)))
        for o in self._dynamic:   # Solver.cpp:249-254 (LDLT: "No collisions with LDLT solver") is checked by the library
            check(lib().admm_hip_add_dynamic_tetmesh(ctx, o.vert_offset, o.rest.shape[0], dptr(o.rest), o.tets.shape[0],
                                                     iptr(o.tets), o.faces.shape[0], iptr(o.faces)))
        if s.soft_modes > 0 and s.linsolver != 1 and not (s.world_size > 1 and os.environ.get("ADMM_HIP_DIST_SOLVE") == "1"):
            check(lib().admm_hip_compute_soft_modes(ctx, int(s.soft_modes), 0))
        if s.monitor:
            check(lib().admm_hip_set_monitor(ctx, int(s.monitor)))
        if s.admm_tol != 0.0 or s.admm_min_iters != 1:
            check(lib().admm_hip_set_admm_stop(ctx, float(s.admm_tol), int(s.admm_min_iters)))
        if s.anderson:
            check(lib().admm_hip_set_anderson(ctx, int(s.anderson)))
        self.initialized = True
        return True

    # ---- Solver::step (src/Solver.cpp:35-110) ------------------------------------------------------
    def step(self):
        """One time step on the host-visible state m_x/m_v (uploaded, stepped on the GPU, downloaded)."""
        self.upload()
        self.step_device(stats=True)
        self.download()

    def upload(self):
        self._need_ctx()
        self.m_x = f64(self.m_x); self.m_v = f64(self.m_v)
        check(lib().admm_hip_set_state(self._ctx, dptr(self.m_x), dptr(self.m_v)))

    def download(self):
        self._need_ctx()
        check(lib().admm_hip_get_state(self._ctx, dptr(self.m_x), dptr(self.m_v)))

    def step_device(self, stats=False, admm_iters=None):
        """admm_hip_step on the device-resident state (no host<->device copies)."""
        self._need_ctx()
        s = self._settings
        it = s.admm_iters if admm_iters is None else admm_iters
        if stats:
            st = Stats()
            check(lib().admm_hip_step(self._ctx, it, s.gravity, C.byref(st)))
            r = self._runtime = RuntimeData()
            r.global_ms, r.local_ms, r.collision_ms = st.global_ms, st.local_ms, st.collision_ms
            r.inner_iters, r.step_ms, r.last_solve_converged = st.inner_iters, st.step_ms, st.last_solve_converged
            r.rhs_ms, r.unconverged_solves, r.pcg_launched_iters = st.rhs_ms, st.unconverged_solves, st.pcg_launched_iters
            r.local_kernel_ms = st.local_kernel_ms
            r.admm_iters = st.admm_iters
            r.pcg_iters_per_solve = list(st.pcg_iters_per_solve)[:min(st.admm_iters, 64)]
        else:
            check(lib().admm_hip_step(self._ctx, it, s.gravity, None))

    def comm_init(self, dist):
        """Multi-GPU: build the RCCL communicator of this rank's context.  `dist` is an initialised
        torch.distributed (any backend) used only to broadcast the 128-byte RCCL unique id."""
        self._need_ctx()
        s = self._settings
        buf = C.create_string_buffer(128)
        if s.rank == 0:
            check(lib().admm_hip_comm_unique_id(buf))
        obj = [bytes(buf.raw)]
        dist.broadcast_object_list(obj, src=0)
        check(lib().admm_hip_comm_init(self._ctx, obj[0], s.rank, s.world_size))

    def comm_info(self):
        """admm_hip_comm_info: dict(n_ranks, rank, device) -- what RCCL says about the context's communicator, and the context's device."""
        self._need_ctx()
        n = C.c_int32(0); r = C.c_int32(-1); buf = C.create_string_buffer(64)
        check(lib().admm_hip_comm_info(self._ctx, C.byref(n), C.byref(r), buf))
        return dict(n_ranks=n.value, rank=r.value, device=buf.value.decode("ascii", "replace"))

    def set_rhs_allreduce(self, fn):
        """admm_hip_set_rhs_allreduce: the multi-GPU exchange over the caller's own transport instead of RCCL.  fn(buf) must sum
        the numpy array `buf` (a view of the library's pinned host buffer, [3 n_verts]) IN PLACE over all ranks; None removes it."""
        self._need_ctx()
        if fn is None:
            self._ar_cb = capi.ALLREDUCE_FN(0)
        else:
            def cb(user, ptr, n):
                try:
                    fn(np.ctypeslib.as_array(ptr, shape=(n,)))
                    return 0
                except Exception:        # a Python exception must not unwind through the C frames
                    import traceback
                    traceback.print_exc()
                    return 1
            self._ar_cb = capi.ALLREDUCE_FN(cb)      # (kept alive as long as the context may call it)
        check(lib().admm_hip_set_rhs_allreduce(self._ctx, self._ar_cb, None))

    def component_partition(self, world_size, settings=None):
        """admm_host_component_partition: (number of connected components, owning rank of every vertex) -- the multi-GPU
        partition admm_hip_create uses when the scene has at least world_size bodies."""
        d = self.make_desc(settings if settings is not None else self._settings)
        vr = np.zeros(self.m_x.size // 3, np.int32)
        n = lib().admm_host_component_partition(C.byref(d), world_size, iptr(vr))
        return n, vr

    def solve_totals(self):
        """admm_hip_solve_totals: (solves, converged solves, inner iterations) of the on-chip PCG since initialize."""
        self._need_ctx()
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().admm_hip_solve_totals(self._ctx, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    # ---- energy and ADMM residuals on the device (csrc/monitor.hpp) -----------------------------------
    def energy(self, x=None, per_term=False):
        """EnergyTerm::energy (src/EnergyTerm.hpp:142-147) of every term at x (default: the device-resident state), reduced on the
        device: dict(tets, tris, hinges, total); with per_term=True also `terms` [n_tets + n_tris + n_bends] in the order the terms
        were added (tets, tris, hinges).  Pins have no energy."""
        self._need_ctx()
        xc = None if x is None else f64(x).ravel().copy()
        if xc is not None and xc.size != self.m_x.size:
            raise ValueError("energy: x must hold 3 values per node")
        tot = np.zeros(4)
        f = getattr(self, "_flat", None) or self.flatten()
        terms = np.zeros(f["tet_idx"].shape[0] + f["tri_idx"].shape[0] + f["bend_idx"].shape[0]) if per_term else None
        check(lib().admm_hip_energy(self._ctx, dptr(xc), dptr(tot), dptr(terms)))
        out = dict(tets=tot[0], tris=tot[1], hinges=tot[2], total=tot[3])
        if per_term:
            out["terms"] = terms
        return out

    def _state_arg(self, x, who):
        xc = None if x is None else f64(x).ravel().copy()
        if xc is not None and xc.size != self.m_x.size:
            raise ValueError(who + ": x must hold 3 values per node")
        return xc

    def forces(self, x=None):
        """admm_hip_forces: the internal forces f = -dE/dx [n_verts, 3] of the energy energy() sums, at x (default: the device-resident
        state).  Triangles ignore their strain limits, pins add nothing."""
        self._need_ctx()
        xc = self._state_arg(x, "forces")
        f = np.zeros(self.m_x.size)
        check(lib().admm_hip_forces(self._ctx, dptr(xc), dptr(f)))
        return f.reshape(-1, 3)

    def stress(self, x=None):
        """admm_hip_stress: per tet, in the order the tets were added: dict(P [n, 3, 3] = dpsi/dF, stretches [n, 3] (signed),
        von_mises [n] of the Cauchy stress P F^T / J).  At J -> 0 von_mises is what the arithmetic gives."""
        self._need_ctx()
        xc = self._state_arg(x, "stress")
        f = getattr(self, "_flat", None) or self.flatten()
        out = np.zeros((f["tet_idx"].shape[0], 13))
        check(lib().admm_hip_stress(self._ctx, dptr(xc), dptr(out)))
        return dict(P=out[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1).copy(), stretches=out[:, 9:12].copy(), von_mises=out[:, 12].copy())

    def stiffness_apply(self, d, x=None, shift=0.0):
        """admm_hip_stiffness_apply: K(x) d + shift * (m o d) with K = d2E/dx2 = -d forces / dx the tangent stiffness of the energy
        energy() sums, at x (default: the device-resident state); m the nodal masses.  d is [n_verts, 3] or [k, n_verts, 3], the result
        has the same shape; every direction of a stack equals the same direction applied alone, bit for bit.  Sign: the result is
        +K d, so forces(x + e d) = forces(x) - e K d + O(e^2); shift = 1 / dt^2 gives the Jacobian of the implicit-Euler residual that
        `stationarity` measures.  K is exact (not projected to a positive semi-definite matrix, not ADMM's constant matrix).  Limits:
        triangles ignore their strain limits, pins add nothing and are not masked, at a stretch of exactly 0 (a kink of the |sigma|
        kinds), at J -> 0 of the Neo-Hookean kinds and at a collapsed triangle the result is what the arithmetic gives.
        Single-GPU contexts."""
        self._need_ctx()
        xc = self._state_arg(x, "stiffness_apply")
        dc = f64(d).copy()
        nv = self.m_x.size // 3
        if dc.ndim not in (2, 3) or dc.shape[-2:] != (nv, 3) or (dc.ndim == 3 and dc.shape[0] < 1):
            raise ValueError("stiffness_apply: d must be [n_verts, 3] or [k, n_verts, 3]")
        out = np.zeros(dc.shape)
        check(lib().admm_hip_stiffness_apply(self._ctx, dptr(xc), 1 if dc.ndim == 2 else dc.shape[0], dptr(dc), float(shift), dptr(out)))
        return out

    def modes(self, k, x=None, shift=0.0, psd=True, hold_pins=True, tol=1e-8, max_iters=2000, guard=None, init=None):
        """admm_hip_modes: the k lowest eigenpairs of (K(x) + shift M) phi = theta M phi on the free vertices, K the tangent frozen at x
        (default: the device-resident state), by LOBPCG with a Jacobi preconditioner on the device (csrc/modal.hpp); psd, hold_pins as
        in stiffness_apply_ex.  Returns (lam [k] = theta - shift ascending, phi [k, n_verts, 3] M-orthonormal and 0 on held vertices,
        info = dict(iterations, converged, converged_modes, restarts, ended_by in ("tol", "max_iters", "breakdown"), residual [k] =
        |A phi_i - theta_i M phi_i| / (|theta_i| |M phi_i|) formed once more at the end, frequency_hz [k] = sqrt(max(lam, 0)) / 2 pi)).
        guard=None means min(4, 16 - k) extra columns; k + guard <= 16.  init: None (a fixed start block) or [k + guard, n_verts, 3].
        With psd=False the lowest modes of an indefinite state are the negative ones.  A body without held vertices needs shift > 0.
        Bit-reproducible.  Single-GPU contexts."""
        self._need_ctx()
        xc = self._state_arg(x, "modes")
        k = int(k)
        if guard is None:
            guard = max(0, min(4, 16 - k))
        guard = int(guard)
        ic = None
        if init is not None:
            ic = f64(init).copy()
            if ic.shape != (k + guard, self.m_x.size // 3, 3):
                raise ValueError("modes: init must be [k + guard, n_verts, 3]")
        kk = max(k, 1)
        lam = np.zeros(kk); phi = np.zeros((kk, self.m_x.size // 3, 3)); info = np.zeros(4 + kk)
        check(lib().admm_hip_modes(self._ctx, dptr(xc), k, guard, float(shift), (1 if psd else 0) | (2 if hold_pins else 0), float(tol),
                                   int(max_iters), dptr(ic), dptr(lam), dptr(phi), dptr(info)))
        return lam, phi, dict(iterations=int(info[0]), converged=int(info[3]) == 0, converged_modes=int(info[1]), restarts=int(info[2]),
                              ended_by=("tol", "max_iters", "breakdown")[int(info[3])], residual=info[4:].copy(),
                              frequency_hz=np.sqrt(np.maximum(lam, 0.0)) / (2.0 * np.pi))

    def stiffness_apply_ex(self, d, x=None, shift=0.0, psd=False, hold_pins=False, block=False):
        """admm_hip_stiffness_apply_ex: stiffness_apply from the tangent FROZEN at x (csrc/newton.hpp: one setup pass with the SVD, then
        one pass per direction).  psd replaces every element tangent by its nearest positive semi-definite one (an element that is
        positive semi-definite already keeps its bits); hold_pins holds the pinned vertices (the rule of `stationarity`): their rows of
        the result are 0 and d is ignored there.  With neither it is stiffness_apply in another summation order.  Shapes, sign, limits
        and reproducibility as there.  block=True sends all directions through the block pass (one copy up, block passes of up to 16
        directions, one copy back): the same bits.  Single-GPU contexts."""
        self._need_ctx()
        xc = self._state_arg(x, "stiffness_apply_ex")
        dc = f64(d).copy()
        nv = self.m_x.size // 3
        if dc.ndim not in (2, 3) or dc.shape[-2:] != (nv, 3) or (dc.ndim == 3 and dc.shape[0] < 1):
            raise ValueError("stiffness_apply_ex: d must be [n_verts, 3] or [k, n_verts, 3]")
        out = np.zeros(dc.shape)
        check(lib().admm_hip_stiffness_apply_ex(self._ctx, dptr(xc), 1 if dc.ndim == 2 else dc.shape[0], dptr(dc), float(shift),
                                                (1 if psd else 0) | (2 if hold_pins else 0) | (4 if block else 0), dptr(out)))
        return out

    def tangent_solve(self, rhs, x=None, shift=None, psd=True, hold_pins=True, tol=1e-10, max_iters=1000):
        """admm_hip_tangent_solve: y with (K(x) + shift M) y = rhs on the free vertices, by Jacobi-preconditioned CG on the device
        (matrix-free on the frozen tangent; no host synchronisation inside the solve).  shift=None means 1 / dt^2: the Hessian of the
        implicit-Euler objective.  psd, hold_pins as in stiffness_apply_ex (held vertices: y = 0).  Returns (y [n_verts, 3], info) with
        info = dict(iterations, converged, residual = |rhs - A y| / |rhs| of the returned y over the free rows (formed once more at the
        end: not the recursive residual the stop test reads), rhs_norm).  With psd=False the operator can be
        indefinite: the solve then ends with converged=False at the first p.Ap <= 0 and returns the iterate before it."""
        self._need_ctx()
        xc = self._state_arg(x, "tangent_solve")
        rc = f64(rhs).ravel().copy()
        if rc.size != self.m_x.size:
            raise ValueError("tangent_solve: rhs must hold 3 values per node")
        shift = self._shift_or_default(shift)
        y = np.zeros(rc.size); info = np.zeros(4)
        check(lib().admm_hip_tangent_solve(self._ctx, dptr(xc), dptr(rc), float(shift), (1 if psd else 0) | (2 if hold_pins else 0), float(tol),
                                           int(max_iters), dptr(y), dptr(info)))
        return y.reshape(-1, 3), self._solve_info(info)

    def _shift_or_default(self, shift):
        """shift=None: 1 / dt^2, the Hessian of the implicit-Euler objective"""
        return 1.0 / (self._settings.timestep_s ** 2) if shift is None else shift

    @staticmethod
    def _solve_info(row):
        """one row of a solve's info: [iterations, converged, residual, rhs_norm(, stationarity, shift)]"""
        d = dict(iterations=int(row[0]), converged=bool(row[1]), residual=float(row[2]), rhs_norm=float(row[3]))
        if len(row) > 4:
            d.update(stationarity=float(row[4]), shift=float(row[5]))
        return d

    @staticmethod
    def _block_info(cols, binfo):
        return dict(columns=cols, block_iterations=int(binfo[0]), column_passes=int(binfo[1]), blocked=bool(binfo[2]))

    def tangent_solve_block(self, rhs, x=None, shift=None, psd=True, hold_pins=True, tol=1e-10, max_iters=1000):
        """admm_hip_tangent_solve_block: tangent_solve for a stack rhs [k, n_verts, 3] on the same frozen operator -- one setup, one
        diagonal, and k independent CG recurrences that share every launch (csrc/newton.hpp: the block PCG; not a block-Krylov method).
        Column j of the result is tangent_solve(rhs[j]) bit for bit, its info included; a column that has ended costs nothing from the
        next iteration on.  Arguments as tangent_solve.  Returns (Y [k, n_verts, 3], info) with info = dict(columns = [tangent_solve's
        info dict per column], block_iterations = the iterations of the longest column, column_passes = the columns applied over all
        iterations, counted on the device, blocked).  More than 16 columns run in slabs of 16.  With set_tangent_precond("two_level")
        the columns are solved one after the other as tangent_solve solves them and blocked is False."""
        self._need_ctx()
        xc = self._state_arg(x, "tangent_solve_block")
        rc = f64(rhs).copy()
        nv = self.m_x.size // 3
        if rc.ndim != 3 or rc.shape[0] < 1 or rc.shape[1:] != (nv, 3):
            raise ValueError("tangent_solve_block: rhs must be [k, n_verts, 3] with k >= 1")
        k = rc.shape[0]
        shift = self._shift_or_default(shift)
        y = np.zeros(rc.shape); info = np.zeros((k, 4)); binfo = np.zeros(3)
        check(lib().admm_hip_tangent_solve_block(self._ctx, dptr(xc), k, dptr(rc), float(shift), (1 if psd else 0) | (2 if hold_pins else 0),
                                                 float(tol), int(max_iters), dptr(y), dptr(info), dptr(binfo)))
        return y, self._block_info([self._solve_info(i) for i in info], binfo)

    def set_tangent_precond(self, kind="jacobi", aggregates=None):
        """admm_hip_set_tangent_precond: the preconditioner of the CG behind tangent_solve, newton_polish and step_adjoint, from the next
        solve on.  "jacobi" (the default) or "two_level": D^-1 + P (P^T A P)^-1 P^T with the affine displacements of `aggregates` compact
        aggregates of vertices (1 .. 64; None: n_verts / 256 clamped to that range) as the coarse space, rebuilt at the x of every solve.
        Fewer iterations of six launches instead of four, plus a setup of ceil(12 aggregates / 16) block passes and a dense inverse per
        solve.  Single-GPU contexts."""
        self._need_ctx()
        kinds = {"jacobi": 0, "two_level": 1}
        if kind not in kinds:
            raise ValueError("set_tangent_precond: kind is 'jacobi' or 'two_level'")
        check(lib().admm_hip_set_tangent_precond(self._ctx, kinds[kind], 0 if aggregates is None else int(aggregates)))

    def tangent_precond(self):
        """admm_hip_get_tangent_precond: dict(kind, aggregates (0: the default)) and, of the last solve, coarse_dim (0: Jacobi),
        coarse_dropped (columns of the coarse space left out: held aggregates, a flat cloth), coarse_ok (False: the coarse matrix was not
        positive definite and the solve ran as Jacobi-PCG), setup_passes."""
        self._need_ctx()
        v = [C.c_int32(0) for _ in range(6)]
        check(lib().admm_hip_get_tangent_precond(self._ctx, *[C.byref(q) for q in v]))
        return dict(kind=("jacobi", "two_level")[v[0].value], aggregates=v[1].value, coarse_dim=v[2].value, coarse_dropped=v[3].value,
                    coarse_ok=bool(v[4].value), setup_passes=v[5].value)

    def tangent_precond_apply(self, r, x=None, shift=None, psd=True, hold_pins=True):
        """admm_hip_tangent_precond_apply (tests): z = M^-1 r of the two-level preconditioner of the tangent frozen at x, with the
        aggregates set by set_tangent_precond; arguments as tangent_solve."""
        self._need_ctx()
        xc = self._state_arg(x, "tangent_precond_apply")
        rc = f64(r).ravel().copy()
        if rc.size != self.m_x.size:
            raise ValueError("tangent_precond_apply: r must hold 3 values per node")
        shift = self._shift_or_default(shift)
        z = np.zeros(rc.size)
        check(lib().admm_hip_tangent_precond_apply(self._ctx, dptr(xc), dptr(rc), float(shift), (1 if psd else 0) | (2 if hold_pins else 0), dptr(z)))
        return z.reshape(-1, 3)

    def set_tangent_coarse(self, solver="one_block"):
        """admm_hip_set_tangent_coarse: the dense inverse of the coarse matrix behind the two-level preconditioner, from the next solve on.
        "one_block" (the default): one workgroup on the matrix in global memory.  "blocked": a tiled Cholesky and a tiled L^-T L^-1 in
        64 x 64 tiles held in LDS, one launch per phase spread over the chip; the same rules for dropped columns and for a matrix that is
        not positive definite, the two inverses differ by rounding.  Single-GPU contexts."""
        self._need_ctx()
        solvers = {"one_block": 0, "blocked": 1}
        if solver not in solvers:
            raise ValueError("set_tangent_coarse: solver is 'one_block' or 'blocked'")
        check(lib().admm_hip_set_tangent_coarse(self._ctx, solvers[solver]))

    def tangent_coarse(self):
        """admm_hip_get_tangent_coarse: dict(solver, tile (of the blocked inverse), launches (kernel launches of the last inverse: the
        setup of the last two-level solve, or a later tangent_coarse_invert)))."""
        self._need_ctx()
        v = [C.c_int32(0) for _ in range(3)]
        check(lib().admm_hip_get_tangent_coarse(self._ctx, *[C.byref(q) for q in v]))
        return dict(solver=("one_block", "blocked")[v[0].value], tile=v[1].value, launches=v[2].value)

    def tangent_coarse_invert(self, A):
        """admm_hip_tangent_coarse_invert (tests): the selected inverse on the device of a symmetric A [n, n], 1 <= n <= 768 ->
        (X, ok, dropped); ok False: A is not positive definite (or not finite) and X = 0."""
        self._need_ctx()
        Ac = np.ascontiguousarray(f64(A))
        if Ac.ndim != 2 or Ac.shape[0] != Ac.shape[1] or not 1 <= Ac.shape[0] <= 768:
            raise ValueError("tangent_coarse_invert: A must be [n, n] with 1 <= n <= 768")
        X = np.zeros_like(Ac)
        ok = C.c_int32(0); dropped = C.c_int32(0)
        check(lib().admm_hip_tangent_coarse_invert(self._ctx, int(Ac.shape[0]), dptr(Ac), dptr(X), C.byref(ok), C.byref(dropped)))
        return X, bool(ok.value), int(dropped.value)

    @staticmethod
    def tangent_plan(xyz, aggregates):
        """admm_host_tangent_plan (no GPU): the aggregates of the two-level tangent preconditioner for the rest positions xyz
        [n_verts, 3] -> (agg_ptr [G + 1], agg_vert [n_verts])."""
        xc = f64(xyz).reshape(-1, 3).copy()
        G = int(aggregates)
        ptr = np.zeros(max(G, 0) + 1, np.int32); vert = np.zeros(max(len(xc), 1), np.int32)
        check(lib().admm_host_tangent_plan(len(xc), dptr(xc), G, iptr(ptr), iptr(vert)))
        return ptr, vert[:len(xc)]

    def newton_polish(self, max_iters=10, grad_tol=1e-8, cg_tol=1e-8, cg_max=500):
        """admm_hip_newton_polish: projected Newton with a backtracking line search on the objective of the last step, applied to the
        device-resident state; m_x and m_v are downloaded afterwards.  Returns one dict per iterate (the first is the state the step left):
        objective, grad_norm (|g| over the free rows: the `stationarity` of that iterate), cg_iterations and step (of the Newton step
        taken from that iterate; 0, 0.0: none), energy.  grad_tol is absolute, in the units of a force.  Refused for multi-GPU contexts,
        contexts with colliders, strain-limited triangles or slide pins, and before the first step."""
        self._need_ctx()
        cap = int(max_iters) + 1
        rec = np.zeros((cap, 5)); n = C.c_int32(0)
        check(lib().admm_hip_newton_polish(self._ctx, int(max_iters), float(grad_tol), float(cg_tol), int(cg_max), cap, C.byref(n), dptr(rec)))
        self.download()
        return [dict(objective=r[0], grad_norm=r[1], cg_iterations=int(r[2]), step=r[3], energy=r[4]) for r in rec[:min(n.value, cap)]]

    def param_sensitivity(self, a, x=None):
        """admm_hip_param_sensitivity: a^T d forces / d theta per energy term at x (default: the device-resident state), theta what a
        user tunes (csrc/adjoint.hpp: k_param_sens).  a is [n_verts, 3] or [k, n_verts, 3]; returns dict(tets [.., n_tets, 4] = (d_mu,
        d_la, d_kappa, d_scale), tris [.., n_tris], hinges [.., n_bends]) in the order the terms were added, with the leading axis of a.
        With F = U diag(sigma) V^T, sg_i = s_i dpsi/de_i and A^ = U^T Ds(a) Binv V:  d_scale = a . f_e = -vol sum_i sg_i A^_ii (the
        derivative in a factor on the tet's energy) and d_theta = -vol sum_i (d sg_i / d theta) A^_ii for the tet's stored mu, lambda
        and kappa; sg is linear in them, so mu d_mu + la d_la + kappa d_kappa = d_scale for the six kinds that have them.  The linear
        tet and the tabulated spline have none on the device: their three columns are exactly 0 (linear tet: d/dk_bulk = d_scale / k).
        tris and hinges: sum_c a_c . f_{e,c}, the derivative in a factor on the term's energy (w^2; the hinge stiffness).  Sums over
        groups of terms, such as one mu per add_tets call, are the caller's np.bincount over the per-term output.  Every column of a
        stack equals that column alone, bit for bit.  Limits as forces(): kinks of the |sigma| kinds at a stretch of 0, J -> 0,
        strain limits ignored.  Single-GPU contexts."""
        self._need_ctx()
        xc = self._state_arg(x, "param_sensitivity")
        ac = f64(a).copy()
        nv = self.m_x.size // 3
        if ac.ndim not in (2, 3) or ac.shape[-2:] != (nv, 3) or (ac.ndim == 3 and ac.shape[0] < 1):
            raise ValueError("param_sensitivity: a must be [n_verts, 3] or [k, n_verts, 3]")
        f = getattr(self, "_flat", None) or self.flatten()
        lead = ac.shape[:-2]
        tets = np.zeros(lead + (f["tet_idx"].shape[0], 4)); tris = np.zeros(lead + (f["tri_idx"].shape[0],))
        hinges = np.zeros(lead + (f["bend_idx"].shape[0],))
        check(lib().admm_hip_param_sensitivity(self._ctx, dptr(xc), 1 if ac.ndim == 2 else ac.shape[0], dptr(ac), dptr(tets), dptr(tris), dptr(hinges)))
        return dict(tets=tets, tris=tris, hinges=hinges)

    def rest_sensitivity(self, a, x=None):
        """admm_hip_rest_sensitivity: d(a . forces)/dX per rest vertex at x (default: the device-resident state), X the rest positions
        behind add_tets(verts, ...), masses and material constants held fixed (csrc/adjoint.hpp: k_rest_sens).  a is [n_verts, 3] or
        [k, n_verts, 3]; the result has the shape of a.  Per tet, with Binv = Dm^-1, F = Ds(x) Binv, P = dpsi/dF, A = Ds(a) Binv and
        T = H[A] the exact element tangent on A:  d(a . f_e)/dDm = Gs Binv^T,  Gs = -vol [(P : A) I - F^T T - A^T P]; rest corner m + 1
        gets column m, corner 0 minus their sum.  The columns sum to 0 over the vertices (a translation of the rest shape changes
        nothing), and at x = X the result is stiffness_apply(a).  With a = lam of step_adjoint it is the rest-shape gradient of the
        loss; masses lumped from the rest volumes chain through meshes.lumped_masses_tets_grad.  Every column of a stack equals that
        column alone, bit for bit.  Limits as stiffness_apply().  Refused for multi-GPU contexts and for contexts that hold triangles
        or hinges (their rest positions do not reach the library)."""
        self._need_ctx()
        xc = self._state_arg(x, "rest_sensitivity")
        ac = f64(a).copy()
        nv = self.m_x.size // 3
        if ac.ndim not in (2, 3) or ac.shape[-2:] != (nv, 3) or (ac.ndim == 3 and ac.shape[0] < 1):
            raise ValueError("rest_sensitivity: a must be [n_verts, 3] or [k, n_verts, 3]")
        out = np.zeros(ac.shape)
        check(lib().admm_hip_rest_sensitivity(self._ctx, dptr(xc), 1 if ac.ndim == 2 else ac.shape[0], dptr(ac), dptr(out)))
        return out

    def step_adjoint(self, dL_dx, dL_dv=None, psd=False, tol=1e-10, max_iters=2000, params=True, rest=False, held=False):
        """admm_hip_step_adjoint: the adjoint of the last step at the device-resident state.  A converged step satisfies on the free rows
        r = m o (x - x_bar) / dt^2 - f(x; theta) = 0 with x_bar = x_prev + dt v_prev + dt^2 a_ext and v = (x - x_prev) / dt.  For a loss
        L(x, v) with dL_dx = dL/dx and dL_dv = dL/dv (None: 0), both [n_verts, 3]:
            g_x = dL_dx + dL_dv / dt (held rows 0);  A lam = g_x,  A = K(x) + M / dt^2 on the free rows, lam = 0 on held rows
            xbar = dL/dx_bar = m o lam / dt^2        x_prev = dL/dx_prev = m o lam / dt^2 - dL_dv / dt (held rows 0)
            v_prev = dL/dv_prev = m o lam / dt       masses = dL/dm = -lam o (x - x_bar) / dt^2, per degree of freedom, x_bar held fixed
            tets, tris, hinges = lam^T d forces / d theta, as param_sensitivity(lam) lays them out (params=True, else None)
        Returns dict(lam, xbar, x_prev, v_prev, masses [n_verts, 3] each, tets, tris, hinges, info = dict(iterations, converged,
        residual = |g_x - A lam| / |g_x| formed once more at the end, rhs_norm = |g_x|, stationarity = |r_free| of the state -- the
        adjoint means something at a converged state only, see newton_polish -- and shift = 1 / dt^2)).  x_prev and v_prev of one call are
        the dL_dx and dL_dv contributions of the step before it: that is how several steps chain (add the loss's own terms of that
        frame).  Group sums, such as one mu per add_tets call, are the caller's np.bincount over the per-term output.  The solve is
        tangent_solve's (Jacobi-PCG on the device, no host synchronisation inside).  psd=False is the exact tangent, the Jacobian,
        positive definite on the free rows at a minimum; a CG breakdown ends with converged=False.  The state is not changed.  Limits
        as forces(): kinks of the |sigma| kinds, J -> 0, strain limits ignored.  Refused for multi-GPU contexts, contexts with
        colliders, strain-limited triangles or slide pins, and before the first step.
        rest=True adds rest = rest_sensitivity(lam) at the device state, dL/dX of the tets' rest positions [n_verts, 3] (refused as
        rest_sensitivity is); held=True adds held = dL/dx of the held vertices, (dL_dx + dL_dv / dt) - K(x) lam on the held rows and 0
        on the free ones (admm_hip_adjoint_held: K the exact tangent without the mass shift; any terms).  With both off the call and
        its result are what they were."""
        self._need_ctx()
        n3 = self.m_x.size
        gx = f64(dL_dx).ravel().copy()
        gv = None if dL_dv is None else f64(dL_dv).ravel().copy()
        if gx.size != n3 or (gv is not None and gv.size != n3):
            raise ValueError("step_adjoint: dL_dx and dL_dv must hold 3 values per node")
        f = getattr(self, "_flat", None) or self.flatten()
        vec = [np.zeros(n3) for _ in range(5)]
        tets = np.zeros((f["tet_idx"].shape[0], 4)) if params else None
        tris = np.zeros(f["tri_idx"].shape[0]) if params else None
        hinges = np.zeros(f["bend_idx"].shape[0]) if params else None
        info = np.zeros(6)
        check(lib().admm_hip_step_adjoint(self._ctx, dptr(gx), dptr(gv), (1 if psd else 0) | (2 if params else 0), float(tol), int(max_iters),
                                          dptr(vec[0]), dptr(vec[1]), dptr(vec[2]), dptr(vec[3]), dptr(vec[4]), dptr(tets), dptr(tris),
                                          dptr(hinges), dptr(info)))
        lam, xbar, xprev, vprev, mass = (q.reshape(-1, 3) for q in vec)
        out = dict(lam=lam, xbar=xbar, x_prev=xprev, v_prev=vprev, masses=mass, tets=tets, tris=tris, hinges=hinges,
                   info=self._solve_info(info))
        if rest:
            out["rest"] = self.rest_sensitivity(lam)
        if held:
            h = np.zeros(n3)
            check(lib().admm_hip_adjoint_held(self._ctx, dptr(vec[0]), dptr(gx), dptr(gv), dptr(h)))
            out["held"] = h.reshape(-1, 3)
        return out

    def step_adjoint_block(self, dL_dx, dL_dv=None, psd=False, tol=1e-10, max_iters=2000, params=True, rest=False, held=False):
        """admm_hip_step_adjoint_block: step_adjoint for k losses at the same state, dL_dx and dL_dv (None: 0) [k, n_verts, 3].  |r_free|
        of the state is formed once, the k solves are tangent_solve_block's, the parameter sensitivities come from one pass over the
        stack of lam.  Returns step_adjoint's dict with a leading axis k on every array (lam, xbar, x_prev, v_prev, masses
        [k, n_verts, 3]; tets [k, n_tets, 4], tris [k, n_tris], hinges [k, n_bends], or None without params) and info = dict(columns =
        [step_adjoint's info dict per loss], block_iterations, column_passes, blocked) as tangent_solve_block reports them.  Entry j
        equals step_adjoint(dL_dx[j], dL_dv[j]) bit for bit.  rest=True adds rest = rest_sensitivity of the lam stack, held=True adds
        held [k, n_verts, 3] through admm_hip_adjoint_held per loss.  Refused as step_adjoint."""
        self._need_ctx()
        nv = self.m_x.size // 3
        gx = f64(dL_dx).copy()
        gv = None if dL_dv is None else f64(dL_dv).copy()
        if gx.ndim != 3 or gx.shape[0] < 1 or gx.shape[1:] != (nv, 3) or (gv is not None and gv.shape != gx.shape):
            raise ValueError("step_adjoint_block: dL_dx and dL_dv must be [k, n_verts, 3] with k >= 1")
        k = gx.shape[0]
        f = getattr(self, "_flat", None) or self.flatten()
        vec = [np.zeros(gx.shape) for _ in range(5)]
        tets = np.zeros((k, f["tet_idx"].shape[0], 4)) if params else None
        tris = np.zeros((k, f["tri_idx"].shape[0])) if params else None
        hinges = np.zeros((k, f["bend_idx"].shape[0])) if params else None
        info = np.zeros((k, 6)); binfo = np.zeros(3)
        check(lib().admm_hip_step_adjoint_block(self._ctx, k, dptr(gx), dptr(gv), (1 if psd else 0) | (2 if params else 0), float(tol),
                                                int(max_iters), dptr(vec[0]), dptr(vec[1]), dptr(vec[2]), dptr(vec[3]), dptr(vec[4]), dptr(tets),
                                                dptr(tris), dptr(hinges), dptr(info), dptr(binfo)))
        cols = [self._solve_info(i) for i in info]
        out = dict(lam=vec[0], xbar=vec[1], x_prev=vec[2], v_prev=vec[3], masses=vec[4], tets=tets, tris=tris, hinges=hinges,
                   info=self._block_info(cols, binfo))
        if rest:
            out["rest"] = self.rest_sensitivity(vec[0])
        if held:
            h = np.zeros(gx.shape)
            for j in range(k):
                check(lib().admm_hip_adjoint_held(self._ctx, dptr(vec[0][j]), dptr(gx[j]), None if gv is None else dptr(gv[j]), dptr(h[j])))
            out["held"] = h
        return out

    def residuals(self, x, z, z_prev):
        """admm_hip_residuals: (|W(Dx - z)|, |W(z - z_prev)|, |W z|, |W D x|) with z, z_prev in the reference's row layout (num_rows())."""
        self._need_ctx()
        R = self.num_rows()
        x = f64(x).ravel().copy(); z = f64(z).ravel().copy(); zp = f64(z_prev).ravel().copy()
        if x.size != self.m_x.size or z.size != R or zp.size != R:
            raise ValueError("residuals: x needs 3 values per node, z and z_prev num_rows() values")
        out = np.zeros(4)
        check(lib().admm_hip_residuals(self._ctx, dptr(x), dptr(z), dptr(zp), dptr(out)))
        return tuple(out)

    def set_monitor(self, mode):
        """admm_hip_set_monitor: 0 off, 1 residuals, 2 residuals + objective, 3 = 2 + stationarity per ADMM iteration; in effect from
        the next step."""
        self._need_ctx()
        check(lib().admm_hip_set_monitor(self._ctx, int(mode)))
        self._settings.monitor = int(mode)

    def set_admm_stop(self, tol, min_iters=1):
        """admm_hip_set_admm_stop: end a step's ADMM loop after the iteration s (s + 1 >= min_iters) whose record meets
        primal <= tol max(wz, wdx) and dz <= tol wz; tol = 0 switches it off.  In effect from the next step."""
        self._need_ctx()
        check(lib().admm_hip_set_admm_stop(self._ctx, float(tol), int(min_iters)))
        self._settings.admm_tol, self._settings.admm_min_iters = float(tol), int(min_iters)

    def admm_stop(self):
        """admm_hip_get_admm_stop: dict(tol, min_iters, last_iters = ADMM iterations the last step executed, on_device = 1 when the
        remaining ones were skipped on the device, 0 when the host decided or the feature is off)."""
        self._need_ctx()
        t = C.c_double(0.0); m = C.c_int32(0); n = C.c_int32(0); d = C.c_int32(0)
        check(lib().admm_hip_get_admm_stop(self._ctx, C.byref(t), C.byref(m), C.byref(n), C.byref(d)))
        return dict(tol=t.value, min_iters=m.value, last_iters=n.value, on_device=d.value)

    def admm_history(self):
        """Records of the last step (admm_hip_get_monitor), one entry per ADMM iteration, taken after its global solve: dict of arrays
        primal = |W(Dx - z)|, dz = |W(z - z_prev)|, wz = |W z|, wdx = |W D x|, energy, inertia = 1/(2 dt^2) |x - x_bar|^2_M,
        objective = energy + inertia (the last three zero in mode 1), stationarity = |(M (x - x_bar) / dt^2 + grad E(x))_free| over the
        vertices without an active pin (mode 3, zero otherwise).  Empty arrays when the step ran with the monitor off."""
        self._need_ctx()
        n = C.c_int32(0)
        check(lib().admm_hip_get_monitor(self._ctx, 0, C.byref(n), None))
        rec = np.zeros((n.value, 8))
        if n.value:
            check(lib().admm_hip_get_monitor(self._ctx, n.value, C.byref(n), dptr(rec)))
        keys = ("primal", "dz", "wz", "wdx", "energy", "inertia", "objective", "stationarity")
        return {k: rec[:, i].copy() for i, k in enumerate(keys)}

    def set_anderson(self, window):
        """admm_hip_set_anderson: Anderson acceleration of a step's ADMM loop over the newest window + 1 accepted evaluations of the
        fixed-point map (x, u) -> (x after the global solve, u after the local step), safeguarded on the residual; window 0 switches it
        off, 8 is the largest.  In effect from the next step.  linsolver 0, single-GPU contexts without colliders."""
        self._need_ctx()
        check(lib().admm_hip_set_anderson(self._ctx, int(window)))
        self._settings.anderson = int(window)

    def anderson_history(self):
        """Records of the last step (admm_hip_get_anderson), one entry per executed ADMM iteration: dict of arrays accepted, accelerated
        (the iteration started from an extrapolated state), entries (the ring after the evaluation; 0 after a rejection or a cleared
        ring), resid = |F_k| and theta [n][8] (zeros beyond entries - 1).  Empty arrays when the step ran with the window 0."""
        self._need_ctx()
        n = C.c_int32(0)
        check(lib().admm_hip_get_anderson(self._ctx, 0, C.byref(n), None))
        rec = np.zeros((n.value, 12))
        if n.value:
            check(lib().admm_hip_get_anderson(self._ctx, n.value, C.byref(n), dptr(rec)))
        return dict(accepted=rec[:, 0].astype(np.int32), accelerated=rec[:, 1].astype(np.int32), entries=rec[:, 2].astype(np.int32),
                    resid=rec[:, 3].copy(), theta=rec[:, 4:12].copy())

    def set_solver_params(self, kind, max_iters=0, tol=-1.0, omega=0.0):
        """admm_hip_set_solver_params: the LinearSolver objects' public tuning members after initialize (the reference reads them on
        every solve: src/NodalMultiColorGS.hpp:40-46,100, src/UzawaCG.hpp:44-45,92).  kind = LS_NCMCGS (max_iters, tol, omega),
        LS_UZAWACG (max_iters, tol) or LS_LDLT (the PCG standing for the prefactored solve); values <= 0 (tol < 0) keep the current one."""
        self._need_ctx()
        check(lib().admm_hip_set_solver_params(self._ctx, int(kind), int(max_iters), float(tol), float(omega)))

    def solver_params(self, kind):
        """admm_hip_get_solver_params: (max_iters, tol, omega) in effect for that solver."""
        self._need_ctx()
        it = C.c_int32(0); t = C.c_double(0.0); o = C.c_double(0.0)
        check(lib().admm_hip_get_solver_params(self._ctx, int(kind), C.byref(it), C.byref(t), C.byref(o)))
        return it.value, t.value, o.value

    def set_soft_modes(self, Z):
        """admm_hip_set_soft_modes: Z [k, n_verts] (or None): every PCG solve ends with the exact Galerkin projection of its residual on them."""
        self._need_ctx()
        if Z is None or len(Z) == 0:
            check(lib().admm_hip_set_soft_modes(self._ctx, 0, None)); return
        Zc = f64(Z).reshape(len(Z), -1)
        check(lib().admm_hip_set_soft_modes(self._ctx, Zc.shape[0], dptr(Zc)))

    def compute_soft_modes(self, k, iters=0):
        """admm_hip_compute_soft_modes: the library computes the k lowest modes itself and installs them."""
        self._need_ctx()
        check(lib().admm_hip_compute_soft_modes(self._ctx, int(k), int(iters)))

    def get_soft_modes(self):
        """admm_hip_get_soft_modes: Z [k, n_verts] in effect (k = 0: none)."""
        self._need_ctx()
        k = C.c_int32(0)
        check(lib().admm_hip_get_soft_modes(self._ctx, C.byref(k), None))
        Z = np.zeros((k.value, self.m_x.size // 3))
        if k.value:
            check(lib().admm_hip_get_soft_modes(self._ctx, C.byref(k), dptr(Z)))
        return Z

    def soft_modes(self, k, iters=8, seed=0):
        """The k lowest eigenvectors of K = diag(m) + Ahat by inverse subspace iteration on the context's own solver (three right-hand sides
        per global solve) with Rayleigh-Ritz steps on the host; returns (eigenvalues, Z [k, n_verts])."""
        import scipy.sparse as sp
        self._need_ctx()
        rp, ci, va = self.system_matrix()
        nv = self.m_x.size // 3
        K = (sp.csr_matrix((va, ci, rp), shape=(nv, nv)) + sp.diags(f64(self.m_masses)[0::3])).tocsr()
        k3 = 3 * ((k + 2) // 3)
        X = np.random.default_rng(seed).standard_normal((nv, k3))
        ew = np.zeros(k3)
        for it in range(iters):
            X, _ = np.linalg.qr(X)
            Y = np.empty_like(X)
            for c0 in range(0, k3, 3):
                y, _ = self.global_solve(np.ascontiguousarray(X[:, c0:c0 + 3]).ravel(), np.zeros(3 * nv))
                Y[:, c0:c0 + 3] = y.reshape(-1, 3)
            Q, _ = np.linalg.qr(Y)
            H = Q.T @ (K @ Q)
            ew, V = np.linalg.eigh(0.5 * (H + H.T))
            X = Q @ V
        return ew[:k], np.ascontiguousarray(X[:, :k].T)

    def contact_totals(self):
        """admm_hip_contact_totals: rows of C over all UzawaCG solves / rows projected onto an obstacle over all GS sweeps, since initialize."""
        self._need_ctx()
        n = C.c_int64(0)
        check(lib().admm_hip_contact_totals(self._ctx, C.byref(n)))
        return n.value

    def persistent_launches(self):
        """admm_hip_persistent_launches: dict(pcg, gs, schur) -- launches of the persistent solver kernels since initialize."""
        self._need_ctx()
        a = [C.c_int64(0) for _ in range(3)]
        check(lib().admm_hip_persistent_launches(self._ctx, *[C.byref(x) for x in a]))
        return dict(zip(("pcg", "gs", "schur"), (x.value for x in a)))

    def pcg_findings(self):
        """admm_hip_pcg_findings: dict(smoother_given_up, trust_revoked, failed_checks) -- what the on-chip PCG holds against this context."""
        self._need_ctx()
        a = C.c_int32(0); b = C.c_int32(0); n = C.c_int64(0)
        check(lib().admm_hip_pcg_findings(self._ctx, C.byref(a), C.byref(b), C.byref(n)))
        return dict(smoother_given_up=bool(a.value), trust_revoked=bool(b.value), failed_checks=n.value)

    def pcg_instances(self):
        """admm_hip_pcg_instances: dict(last, hot, generic, lane_hot, lane_generic, last_verifications) -- which instance of the on-chip PCG
        kernel served the last solve on the context's own stream ('none', 'generic', 'hot'), the launches of each since initialize, and how
        often that last solve verified its true residual (-1: no solve yet)."""
        self._need_ctx()
        last = C.c_int32(0); n = (C.c_int64 * 4)(); v = C.c_int32(0)
        check(lib().admm_hip_pcg_instances(self._ctx, C.byref(last), n, C.byref(v)))
        return dict(last=("none", "generic", "hot")[last.value], hot=n[0], generic=n[1], lane_hot=n[2], lane_generic=n[3], last_verifications=v.value)

    def pcg_plan(self):
        """admm_hip_pcg_plan_info: dict(enabled, G, spb, T, two_level, handoff, nbr_max, gave_up) -- the plan of the on-chip PCG this context
        runs on: whether it serves the solves, its grid and block shape, the two-level preconditioner, whether the vector exchanges go by
        the neighbour hand-off lists (False: by grid barriers), the most neighbour blocks of a block (-1: more than 64), and whether the
        context gave the persistent kernels up after a time-out."""
        self._need_ctx()
        o = (C.c_int64 * 8)()
        check(lib().admm_hip_pcg_plan_info(self._ctx, o))
        return dict(enabled=bool(o[0]), G=o[1], spb=o[2], T=o[3], two_level=bool(o[4]), handoff=bool(o[5]), nbr_max=o[6], gave_up=bool(o[7]))

    def probe_sync(self, n=200):
        """admm_hip_probe_sync: (us per all-to-all, us per vector exchange, plan statistics dict) of the on-chip PCG."""
        self._need_ctx()
        a = C.c_double(0.0); b = C.c_double(0.0); st = (C.c_int64 * 6)()
        check(lib().admm_hip_probe_sync(self._ctx, n, C.byref(a), C.byref(b), st))
        keys = ("nnz", "stored", "on_chip", "block_local", "max_neighbour_blocks", "coarse_unknowns")
        return a.value, b.value, dict(zip(keys, list(st)))

    def time_local_launches(self, on=True):
        """admm_hip_time_local_launches: event pairs around the local-step launches of the steps issued without statistics
        (on = 2: attached to the dominant local-step kernel's own dispatch)."""
        self._need_ctx()
        check(lib().admm_hip_time_local_launches(self._ctx, int(on) if on in (0, 1, 2) else (1 if on else 0)))

    def local_launch_times(self):
        """admm_hip_local_launch_times: (pairs recorded since the last call, sum of their intervals in ms)."""
        self._need_ctx()
        n = C.c_int64(0); ms = C.c_double(0.0)
        check(lib().admm_hip_local_launch_times(self._ctx, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def uzawa_cache_stats(self):
        """admm_hip_uzawa_cache_stats: dict(columns, column_solves, schur_from_columns, schur_by_pcg, evicted)."""
        self._need_ctx()
        a = [C.c_int64(0) for _ in range(5)]
        check(lib().admm_hip_uzawa_cache_stats(self._ctx, *[C.byref(x) for x in a]))
        d = dict(zip(("columns", "column_solves", "schur_from_columns", "schur_by_pcg", "evicted"), (x.value for x in a)))
        u = C.c_int64(0)
        check(lib().admm_hip_uzawa_unconverged_columns(self._ctx, C.byref(u)))
        d["unconverged_columns"] = u.value
        nb, nl, na, nw = C.c_int64(0), C.c_int(0), C.c_int64(0), C.c_int64(0)
        check(lib().admm_hip_uzawa_column_lanes(self._ctx, C.byref(nb), C.byref(nl), C.byref(na), C.byref(nw)))
        d["lane_batches"], d["lanes"], d["ahead_columns"], d["ahead_waits"] = nb.value, nl.value, na.value, nw.value
        return d

    def tet_rest_mode(self):
        """admm_hip_tet_rest_mode: 0 = the local step streams Binv, 1 / 2 = it recomputes Binv from gathered rest positions."""
        self._need_ctx()
        return lib().admm_hip_tet_rest_mode(self._ctx)

    def runtime_data(self):
        return self._runtime

    def settings(self):
        return self._settings

    # ---- kernel-level entry points (parity tests) -------------------------------------------------
    def num_rows(self):
        self._need_ctx()
        return lib().admm_hip_num_rows(self._ctx)

    def local_step(self, x, u, Mxbar=None):
        """EnergyTerm::update over all terms. Returns (z, u_new[, b])."""
        self._need_ctx()
        R = self.num_rows()
        x = f64(x).ravel().copy(); u = f64(u).ravel().copy()
        assert u.size == R
        z = np.zeros(R)
        b = np.zeros(x.size) if Mxbar is not None else None
        mx = f64(Mxbar).ravel().copy() if Mxbar is not None else None
        check(lib().admm_hip_local_step(self._ctx, dptr(x), dptr(u), dptr(z), dptr(mx), dptr(b)))
        return (z, u, b) if Mxbar is not None else (z, u)

    def regather_rhs(self, u_before=None, reference=False, stop_word=False):
        """admm_hip_regather_rhs (tests): the right-hand side gathered again from what the last local_step left on the device -- by the
        kernel the step launches, or by its reference instantiation (same sums, the loads of a list waited for four records at a time);
        stop_word: the instantiations of a step with the early exit on the device.  u_before: the u handed to that local_step."""
        self._need_ctx()
        u = None if u_before is None else f64(u_before).ravel().copy()
        assert u is None or u.size == self.num_rows()
        b = np.zeros(self.m_x.size)
        check(lib().admm_hip_regather_rhs(self._ctx, dptr(u), (1 if reference else 0) | (2 if stop_word else 0), dptr(b)))
        return b

    def global_solve(self, b, x0):
        """LinearSolver::solve: returns (x, inner_iters)."""
        self._need_ctx()
        b = f64(b).ravel().copy(); x = f64(x0).ravel().copy()
        it = C.c_int32(0)
        check(lib().admm_hip_global_solve(self._ctx, dptr(b), dptr(x), C.byref(it)))
        return x, it.value

    def system_matrix(self):
        """Ahat as (rowptr, col, val): A = diag(m) + Ahat (x) I3."""
        self._need_ctx()
        nnz = C.c_int32(0)
        check(lib().admm_hip_get_matrix(self._ctx, None, None, None, C.byref(nnz)))
        nv = self.m_x.size // 3
        rp = np.zeros(nv + 1, np.int32); ci = np.zeros(nnz.value, np.int32); va = np.zeros(nnz.value)
        check(lib().admm_hip_get_matrix(self._ctx, iptr(rp), iptr(ci), dptr(va), C.byref(nnz)))
        return rp, ci, va

    def gs_colors(self):
        self._need_ctx()
        nv = self.m_x.size // 3
        col = np.zeros(nv, np.int32); nc = C.c_int32(0)
        check(lib().admm_hip_get_colors(self._ctx, iptr(col), C.byref(nc)))
        return col, nc.value

    def _need_ctx(self):
        if not self._ctx:
            raise AdmmHipError(-4, "Solver is not initialized")
