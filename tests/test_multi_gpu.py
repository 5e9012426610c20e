"""The N>1 path: element-block partition, partial right-hand sides, one sum all-reduce per
ADMM iteration, replicated global solve.

  * CPU, world_size 2, gloo: the sharded algorithm (product partition + oracle arithmetic) reproduces
    the single-rank oracle step bit-for-bit up to summation order.
  * GPU (one device): two rank-contexts of a world of 2 produce partial RHS / disjoint z,u rows whose
    union equals the single-context result (everything but the RCCL call itself, which needs >1 GPU).
"""
import os
import socket

import numpy as np
import pytest

import admm_elastic_amd as pkg
from admm_elastic_amd import capi
import scenes


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _worker(rank, world, port, n, frames, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sc = scenes.mixed_cube_scene(n, admm_iters=6, linsolver=0)
    o = sc.make_oracle(mode=1)            # full scene: used for the replicated global solve + matrix
    tb, te = capi.partition(o.nt, world, rank)   # the product's partition rule
    rows = slice(9 * tb, 9 * te)
    Dt = o.DtWtW[:, rows]
    for _ in range(frames):
        # Solver::step with the local step restricted to the owned element block
        o.v[1::3] += o.dt * o.gravity
        x_bar = o.x + o.dt * o.v
        Mxbar = o.m * x_bar
        curr = x_bar.copy()
        z = np.zeros(o.R); u = np.zeros(o.R)
        for _it in range(o.admm_iters):
            zz = np.ascontiguousarray(z[rows]); uu = np.ascontiguousarray(u[rows])
            from oracle import oracle as orc
            orc.lib().orc_local_tets(te - tb, orc._i(np.ascontiguousarray(o.t_idx[tb:te])), orc._p(np.ascontiguousarray(o.t_Binv[tb:te])),
                                     orc._i(np.ascontiguousarray(o.t_kind[tb:te])), orc._p(np.ascontiguousarray(o.t_mu[tb:te])),
                                     orc._p(np.ascontiguousarray(o.t_la[tb:te])), orc._p(np.ascontiguousarray(o.t_k[tb:te])),
                                     orc._p(curr), orc._p(zz), orc._p(uu), 1)
            z[rows] = zz; u[rows] = uu
            part = Dt @ (zz - uu)                       # partial dt^2 D^T W^2 (z - u) of this block
            # pin terms + M x_bar live on rank 0 only
            if rank == 0:
                pr = slice(9 * o.nt, o.R)
                zp = np.ascontiguousarray(z[pr]); up = np.ascontiguousarray(u[pr])
                orc.lib().orc_local_pins(o.npin, orc._i(o.p_vert), orc._p(o.p_xyz), orc._i(o.p_active), orc._p(curr), orc._p(zp), orc._p(up))
                z[pr] = zp; u[pr] = up
                part = part + o.DtWtW[:, pr] @ (zp - up) + Mxbar
            t = torch.from_numpy(part.copy())
            dist.all_reduce(t)                           # the one exchange step per ADMM iteration
            curr = o.solve_ldlt(t.numpy())               # replicated global solve
        o.v = (curr - o.x) / o.dt
        o.x = curr
    if rank == 0:
        q.put(o.x.copy())
    dist.destroy_process_group()


def test_sharded_step_matches_single_rank_gloo():
    import multiprocessing as mp          # (stdlib: the pytest process itself never imports torch -- its bundled ROCm libraries next to the system ones the library loads abort at exit)
    n, frames, world = 4, 3, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, frames, q)) for r in range(world)]
    for p in procs:
        p.start()
    x_sharded = q.get(timeout=300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    sc = scenes.mixed_cube_scene(n, admm_iters=6, linsolver=0)
    o = sc.make_oracle(mode=1)
    for _ in range(frames):
        o.step()
    assert scenes.rel_err(x_sharded, o.x) < 1e-9   # only the summation order of the partial RHS differs


@pytest.mark.gpu
def test_rank_contexts_partition_the_local_step():
    sc = scenes.mixed_cube_scene(5, linsolver=0)
    v2, tris = pkg.meshes.cloth_grid(4, 1.0, 1.3)
    sc.add_tri_mesh(v2, tris, pkg.Lame(100.0, 0.1))
    single = sc.make_solver()
    R = single.num_rows()
    rng = np.random.default_rng(3)
    x = scenes.perturb(sc.x, 0.02, 4).ravel()
    u0 = 0.02 * rng.standard_normal(R); u0[9 * len(single.flatten()["tet_idx"]) + 6 * len(tris):] = 0.0
    Mx = rng.standard_normal(x.size)
    z1, u1, b1 = single.local_step(x, u0, Mx)
    world = 3
    zs = np.zeros(R); us = u0.copy(); bs = np.zeros(x.size)
    touched = np.zeros(R, bool)
    for r in range(world):
        s = sc.make_solver(rank=r, world_size=world)     # no comm_init: local_step returns the PARTIAL b
        z, u, b = s.local_step(x, u0, Mx)
        own = np.abs(z) > 0
        assert not (touched & own)[: 9 * single._flat["tet_idx"].shape[0]].any()
        touched |= own
        zs += z
        us = np.where(u != u0, u, us)
        bs += b
        with pytest.raises(pkg.AdmmHipError):             # stepping a rank context needs the communicator
            s.upload(); s.step_device()
        s.close()
    nrow_el = 9 * single._flat["tet_idx"].shape[0] + 6 * len(tris)
    assert np.abs(zs[:nrow_el] - z1[:nrow_el]).max() < 1e-12
    assert np.abs(us[:nrow_el] - u1[:nrow_el]).max() < 1e-12
    assert np.abs(bs - b1).max() <= 1e-9 * np.abs(b1).max()


@pytest.mark.gpu
def test_world8_rank_contexts_of_the_1m_tet_body_reproduce_the_single_context():
    """BASELINE configs[3] at its size on ONE GPU: the eight rank contexts of the element-block partition of the 1 012 608-tet body
    (bench.py's default workload) against the single context, through the kernel-level entry points -- every ADMM iteration: the eight
    local steps on their element blocks (disjoint z / u rows, partial right-hand sides: rank 0 carries M x_bar and the pin terms), the
    sum of the partials (what the all-reduce does), the replicated solve on rank 0's context.  One frame of 3 ADMM iterations equals
    the single context's frame to the solve tolerance."""
    import bench
    n = int(os.environ.get("ADMM_TEST_BIG_BLOB_N", "118"))
    sc, nt, nv = bench.build_scene(bench.WORKLOADS["blob1m_mix"], n)
    sc.settings.update(admm_iters=3, linsolver=0)
    world, iters = 8, 3
    single = sc.make_solver(pcg_tol=1e-11, pcg_max_iters=2000)
    single.step()
    assert single.runtime_data().unconverged_solves == 0
    ranks = [sc.make_solver(rank=r, world_size=world, pcg_tol=1e-11, pcg_max_iters=2000) for r in range(world)]
    R = ranks[0].num_rows()
    dt, g = sc.settings["timestep_s"], sc.settings["gravity"]
    m = sc.masses3()
    x0 = sc.x.ravel().copy(); v = np.zeros_like(x0); v[1::3] += dt * g
    xbar = x0 + dt * v
    Mxbar = m * xbar
    curr = xbar.copy()
    u = np.zeros(R)
    for it in range(iters):
        b = np.zeros_like(x0); u_new = u.copy(); rows_seen = np.zeros(R, bool)
        for r in range(world):
            z_r, u_r, b_r = ranks[r].local_step(curr, u, Mxbar)
            own = u_r != u
            if it == 0:
                own = np.abs(z_r) > 0
            assert not (rows_seen & own)[:9 * nt].any()      # the ranks' element rows are disjoint (every rank carries the pin rows)
            rows_seen |= own
            u_new = np.where(own, u_r, u_new)
            b += b_r
        u = u_new
        curr, _ = ranks[0].global_solve(b, curr)
    err = scenes.rel_err(curr, single.m_x)
    assert err < 1e-8, err
    assert np.abs(single.m_x - x0).max() > 1e-4
    for s_ in ranks:
        s_.close()
    single.close()


@pytest.mark.gpu
def test_rccl_allreduce_path_on_one_gpu():
    """The RCCL leg of the multi-GPU step on a single GPU: a communicator of world size 1 (ADMM_HIP_FORCE_COMM=1)
    makes every ADMM iteration run the in-place ncclAllReduce of the right-hand side on the context's stream,
    between the gather kernel and the persistent PCG kernel.  The all-reduce over one rank is the identity, so
    the trajectory must equal the plain single-GPU one bit for bit."""
    import ctypes as C
    from admm_elastic_amd import capi
    sc = scenes.mixed_cube_scene(6, admm_iters=6, linsolver=0)
    ref = sc.make_solver(pcg_tol=1e-10, pcg_max_iters=500)
    for _ in range(3):
        ref.step()
    s = sc.make_solver(pcg_tol=1e-10, pcg_max_iters=500)
    os.environ["ADMM_HIP_FORCE_COMM"] = "1"
    try:
        buf = C.create_string_buffer(128)
        capi.check(capi.lib().admm_hip_comm_unique_id(buf))
        capi.check(capi.lib().admm_hip_comm_init(s._ctx, bytes(buf.raw), 0, 1))
    finally:
        os.environ.pop("ADMM_HIP_FORCE_COMM", None)
    for _ in range(3):
        s.step()
    assert np.array_equal(s.m_x, ref.m_x)
    assert s.runtime_data().unconverged_solves == 0
    s.close(); ref.close()


@pytest.mark.gpu
def test_distributed_solve_collectives_over_rccl_on_one_gpu(monkeypatch):
    """The RCCL leg of the distributed solve on one GPU: a world of ONE with a communicator and ADMM_HIP_DIST_SOLVE=1 runs every
    collective of launch_pcg_dist (partials, u, x) as an in-place ncclAllReduce on the context's stream; over one rank they are the
    identity and the row range is everything, so the result is the launch-per-iteration solver's, and matches the on-chip one to
    solver tolerance.  (Two ranks: test_distributed_solve_matches_single_context, gloo; two GPUs: test_two_ranks_two_gpus_*.)"""
    import ctypes as C
    sc = scenes.mixed_cube_scene(6, admm_iters=6, linsolver=0)
    ref = sc.make_solver(pcg_tol=1e-12, pcg_max_iters=1000)
    monkeypatch.setenv("ADMM_HIP_FORCE_COMM", "1")
    monkeypatch.setenv("ADMM_HIP_DIST_SOLVE", "1")
    s = sc.make_solver(pcg_tol=1e-12, pcg_max_iters=1000)
    buf = C.create_string_buffer(128)
    capi.check(capi.lib().admm_hip_comm_unique_id(buf))
    capi.check(capi.lib().admm_hip_comm_init(s._ctx, bytes(buf.raw), 0, 1))
    for _ in range(3):
        s.step(); ref.step()
        assert s.runtime_data().unconverged_solves == 0
    assert s.runtime_data().inner_iters > ref.runtime_data().inner_iters      # Jacobi PCG, not the on-chip two-level one: it is the other path
    assert scenes.rel_err(s.m_x, ref.m_x) < 1e-9
    s.close(); ref.close()


def _rccl_worker(rank, world, port, n, frames, q, dist_solve=False):
    """One rank of a real multi-GPU run: own device, RCCL communicator, product contexts."""
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    if dist_solve:
        os.environ["ADMM_HIP_DIST_SOLVE"] = "1"
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)     # only carries the 128-byte RCCL id
    sc = scenes.mixed_cube_scene(n, admm_iters=6, linsolver=0)
    s = sc.make_solver(device=rank, rank=rank, world_size=world, pcg_tol=1e-10, pcg_max_iters=500)
    s.comm_init(dist)
    for _ in range(frames):
        s.step()
    q.put((rank, s.m_x.copy(), s.runtime_data().unconverged_solves))
    dist.barrier()
    s.close()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("dist_solve", [False, True])
def test_two_ranks_two_gpus_match_single_context(dist_solve):
    """A real world-2 step (element-block partition, ncclAllReduce of the partial right-hand side over xGMI between the
    gather kernel and the persistent PCG kernel, replicated solve) on two devices reproduces the single-context
    trajectory; dist_solve: the same with the PCG's rows split over the two devices (ADMM_HIP_DIST_SOLVE=1: RCCL all-reduces of the
    partial sums and of u per PCG iteration).  Needs two GPUs: skipped on the 1-GPU test boxes, run wherever the driver has a
    multi-GPU node."""
    if pkg.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    import multiprocessing as mp          # (stdlib: the pytest process itself never imports torch -- its bundled ROCm libraries next to the system ones the library loads abort at exit)
    n, frames, world = 6, 3, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rccl_worker, args=(r, world, port, n, frames, q, dist_solve)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in range(world)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    sc = scenes.mixed_cube_scene(n, admm_iters=6, linsolver=0)
    ref = sc.make_solver(pcg_tol=1e-10, pcg_max_iters=500)
    for _ in range(frames):
        ref.step()
    for rank, x, unconv in res:
        assert unconv == 0
        assert scenes.rel_err(x, ref.m_x) < 1e-9, (rank, scenes.rel_err(x, ref.m_x))   # summation order of the partial RHS differs
    assert np.array_equal(res[0][1], res[1][1])      # the replicated solves see the same all-reduced right-hand side


# ---- component-aware partition: whole bodies per rank, no exchange inside a step (admm_hip_ctx::CompMode) -------------------
def test_component_partition_assigns_whole_bodies():
    """admm_host_component_partition: bodies by decreasing element count to the least loaded rank; a body is never cut; a
    single body gives one component (then admm_hip_create falls back to element blocks)."""
    sc = scenes.bodies_scene([3, 5, 2, 4, 3], linsolver=0)
    s = sc.make_solver(init=False)
    body = np.concatenate([np.full(len(t[0]), i) for i, t in enumerate(sc.tets)])      # body of every vertex
    ntet = np.array([len(t[1]) for t in sc.tets])
    for world in (1, 2, 3, 5):
        n, vr = s.component_partition(world, sc.product_settings)
        assert n == 5
        for b in range(5):
            assert len(set(vr[body == b])) == 1                                        # whole bodies
        rank_of_body = np.array([vr[body == b][0] for b in range(5)])
        load = np.array([ntet[rank_of_body == r].sum() for r in range(world)])
        assert (load > 0).all() and load.max() <= ntet.sum() / world + ntet.max()       # nobody idle, greedy balance
        n2, vr2 = s.component_partition(world, sc.product_settings)
        assert n2 == n and np.array_equal(vr, vr2)                                      # deterministic
    # largest body first to rank 0, the next to rank 1, ...
    n, vr = s.component_partition(2, sc.product_settings)
    assert vr[body == 1][0] == 0 and vr[body == 3][0] == 1
    # loose vertices (no element) are not bodies: one body + 7 loose vertices is ONE component, whatever the world size
    loose = scenes.cube_scene(3, pkg.TET_LINEAR, linsolver=0)
    ls = loose.make_solver(init=False)
    ls.add_nodes(np.arange(21.0).reshape(7, 3) + 5.0, np.ones(21))
    n, vr = ls.component_partition(4, loose.product_settings)
    assert n == 1 and len(vr) == len(loose.x) + 7 and len(set(vr[:len(loose.x)])) == 1
    one = scenes.mixed_cube_scene(4, linsolver=0).make_solver(init=False)
    n, vr = one.component_partition(4, scenes.mixed_cube_scene(4, linsolver=0).make_solver(init=False)._settings)
    assert n == 1 and (vr == 0).all()


def _component_worker(rank, world, port, frames, q):
    """One rank of the component-partitioned job on the CPU: the oracle steps ONLY the bodies admm_host_component_partition gives
    this rank (a sub-scene with its own exact solve -- the rank's block of the block-diagonal system); positions are merged by
    an all-gather at the end, as admm_hip_get_state does with its communicator."""
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ["OMP_NUM_THREADS"] = "2"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sc = scenes.bodies_scene([3, 4, 2], admm_iters=6, linsolver=0)
    n, vr = sc.make_solver(init=False).component_partition(world)
    own = np.nonzero(vr == rank)[0]
    g2l = -np.ones(len(sc.x), np.int64); g2l[own] = np.arange(len(own))
    sub = scenes.Scene()
    sub.x = sc.x[own]; sub.m = sc.m[own]
    for verts, tets, lame, kind, off in sc.tets:
        if vr[off] == rank:
            sub.tets.append((sub.x, g2l[tets + off].astype(np.int32), lame, kind, 0))
    sub.pins = {int(g2l[k]): p for k, p in sc.pins.items() if vr[k] == rank}
    sub.settings.update(sc.settings)
    o = sub.make_oracle(mode=1)
    for _ in range(frames):
        o.step()
    mine = np.zeros(3 * len(sc.x)); mine.reshape(-1, 3)[own] = o.x.reshape(-1, 3)
    t = torch.from_numpy(mine)
    dist.all_reduce(t)                      # merge (every vertex has exactly one owner)
    if rank == 0:
        q.put(t.numpy().copy())
    dist.destroy_process_group()


def test_component_partition_matches_single_rank_gloo():
    import multiprocessing as mp          # (stdlib: the pytest process itself never imports torch -- its bundled ROCm libraries next to the system ones the library loads abort at exit)
    frames, world = 3, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_component_worker, args=(r, world, port, frames, q)) for r in range(world)]
    for p in procs:
        p.start()
    x_merged = q.get(timeout=300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    sc = scenes.bodies_scene([3, 4, 2], admm_iters=6, linsolver=0)
    o = sc.make_oracle(mode=1)
    for _ in range(frames):
        o.step()
    assert scenes.rel_err(x_merged, o.x) < 1e-10      # exact solves of the blocks of a block-diagonal system = the exact solve


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_component_rank_contexts_reproduce_single_context(world):
    """World-N rank contexts on ONE GPU (no communicator): every context holds its rank's bodies only, steps them without any
    exchange, and the merged trajectory is the single context's (to the solve tolerance: the ranks' PCG solves are the blocks of
    the single context's solve).  Pins moved through the global numbering; the kernel-level entry points refuse."""
    sc = scenes.bodies_scene([4, 6, 3, 5], admm_iters=8, linsolver=0)
    frames = 3
    moved = {k: p + np.array([0.02, 0.0, 0.01]) for k, p in sc.pins.items()}
    ref = sc.make_solver(pcg_tol=1e-11, pcg_max_iters=2000)
    for f in range(frames):
        ref.step()
        if f == 0:
            ref.set_pins(list(moved.keys()), list(moved.values()))
    n, vr = ref.component_partition(world)
    assert n == 4
    merged = np.zeros_like(ref.m_x)
    for r in range(world):
        s = sc.make_solver(rank=r, world_size=world, pcg_tol=1e-11, pcg_max_iters=2000)
        x0 = s.m_x.copy()
        for f in range(frames):
            s.step()
            if f == 0:
                s.set_pins(list(moved.keys()), list(moved.values()))
        own = np.repeat(vr == r, 3)
        assert np.array_equal(s.m_x[~own], x0[~own])              # the other ranks' bodies are not touched
        assert s.runtime_data().unconverged_solves == 0
        merged[own] = s.m_x[own]
        with pytest.raises(pkg.AdmmHipError):
            s.local_step(s.m_x, np.zeros(s.num_rows()))
        s.close()
    assert scenes.rel_err(merged, ref.m_x) < 1e-9, scenes.rel_err(merged, ref.m_x)
    assert np.abs(ref.m_x - sc.x.ravel()).max() > 1e-3


@pytest.mark.gpu
def test_component_partition_merges_over_rccl_on_one_gpu(monkeypatch):
    """The RCCL leg of the component partition on one GPU: a world of ONE with ADMM_HIP_PARTITION=components and a communicator:
    admm_hip_get_state runs its merging all-reduce (the identity here) and returns the single-context trajectory bit for bit."""
    import ctypes as C
    sc = scenes.bodies_scene([4, 3], admm_iters=6, linsolver=0)
    ref = sc.make_solver(pcg_tol=1e-10, pcg_max_iters=500)
    for _ in range(3):
        ref.step()
    monkeypatch.setenv("ADMM_HIP_PARTITION", "components")
    s = sc.make_solver(rank=0, world_size=2, pcg_tol=1e-10, pcg_max_iters=500)      # rank 0 of 2: the larger body
    monkeypatch.delenv("ADMM_HIP_PARTITION")
    for _ in range(3):
        s.step()
    n, vr = ref.component_partition(2)
    own = np.repeat(vr == 0, 3)
    single_body = scenes.bodies_scene([4], admm_iters=6, linsolver=0).make_solver(pcg_tol=1e-10, pcg_max_iters=500)
    for _ in range(3):
        single_body.step()
    assert np.array_equal(s.m_x[own], single_body.m_x)        # the rank's context IS the single-GPU solver of its bodies


@pytest.mark.gpu
def test_barrier_timeout_under_a_communicator_is_a_clean_comm_error(monkeypatch):
    """A grid barrier of the persistent PCG kernel that cannot complete is recovered by a replay on a single GPU
    (tests/test_edge_cases.py); under a communicator a replay on one rank would issue all-reduces the others do not, so the
    step fails with ADMM_HIP_ERR_COMM and a message that says what to do -- never a hang, never a wrong state."""
    import ctypes as C
    sc = scenes.mixed_cube_scene(6, admm_iters=6, linsolver=0)
    monkeypatch.setenv("ADMM_HIP_TEST_ABORT_SOLVE", "8")
    s = sc.make_solver(pcg_tol=1e-10, pcg_max_iters=500)
    monkeypatch.delenv("ADMM_HIP_TEST_ABORT_SOLVE")
    monkeypatch.setenv("ADMM_HIP_FORCE_COMM", "1")
    buf = C.create_string_buffer(128)
    capi.check(capi.lib().admm_hip_comm_unique_id(buf))
    capi.check(capi.lib().admm_hip_comm_init(s._ctx, bytes(buf.raw), 0, 1))
    monkeypatch.delenv("ADMM_HIP_FORCE_COMM")
    s.step()
    with pytest.raises(pkg.AdmmHipError) as ei:
        s.step()                                   # solve 8 is in the second frame
    assert ei.value.code == -5 and "communicator" in str(ei.value)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("series", ["strong", "weak"])
def test_bench_two_ranks_share_one_gpu_functional(series):
    """`python bench.py --gpus 2` end to end on a one-GPU box (ADMM_BENCH_SHARE_GPU=1: both ranks on device 0, gloo, the partial
    right-hand sides summed through admm_hip_set_rhs_allreduce because RCCL refuses two ranks on one device).  strong = the DEFAULT
    line: BASELINE configs[3], ONE body at fixed tet count, element-block partition, one all-reduce per ADMM iteration, the weak
    series riding along as `weak_value`; weak = `--workload blobs_1m_per_gpu`, one body per rank, component partition.  A functional
    check of the N-rank code paths -- the two ranks time-share the device, the numbers mean nothing."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ADMM_BENCH_SHARE_GPU="1", ADMM_BENCH_N="30")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"]
    if series == "weak":
        cmd += ["--workload", "blobs_1m_per_gpu"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["scaling"] == series
    assert d["unconverged_solves_in_timed_region"] == 0 and d["finite"] and d["value"] > 0
    if series == "strong":
        assert d["config"]["workload"].startswith("blob1m_mix")
        assert "element-block x2" in d["config"]["parallelism"]
        assert d["weak_value"] > 0 and d["weak"]["expected_vs_one_gpu"] == 2.0
        assert 0.5 < d["expected_speedup"]["vs_one_gpu"] < 2.0 and "single_gpu_ms_per_admm_iter" in d["expected_speedup"]
    else:
        assert d["config"]["workload"].startswith("blobs_1m_per_gpu")
        assert "whole bodies per rank x2" in d["config"]["parallelism"] and d["expected_speedup"]["vs_one_gpu"] == 2.0


@pytest.mark.gpu
@pytest.mark.parametrize("series", ["strong", "weak"])
def test_bench_two_ranks_share_one_gpu_plain_line_and_dump(series, tmp_path):
    """The PLAIN `python bench.py --gpus 2` (no --full) on a one-GPU box, as above: the headline line alone, and --dump-outputs with
    every rank downloading (a collective under the component partition with a communicator).  weak: rank 0's dump holds BOTH bodies
    stepped -- without a communicator each rank fills only its own body, and bench.py merges the two parts."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ADMM_BENCH_SHARE_GPU="1", ADMM_BENCH_N="30")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)]
    if series == "weak":
        cmd += ["--workload", "blobs_1m_per_gpu"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == series and d["steps"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["metric"] == "ADMM iterations/sec" and d["unit"] == "ADMM it/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    for k in ("split_ms_per_admm_iter", "finite", "weak_value", "expected_speedup", "rccl"):
        assert k not in d, k
    nv = d["config"]["verts"]
    x, v = np.load(tmp_path / "m_x.npy"), np.load(tmp_path / "m_v.npy")
    assert x.shape == (nv, 3) and v.shape == (nv, 3) and np.isfinite(x).all() and np.isfinite(v).all()
    halves = (slice(0, nv // 2), slice(nv // 2, nv)) if series == "weak" else (slice(0, nv),)
    for h in halves:                                   # (weak: two copies of one body, body 0 first)
        assert np.abs(v[h]).max() > 0, h
    if series == "weak":                               # the two bodies are the same body 2 m apart, stepped alike
        assert np.abs(x[halves[1]] - np.array([2.0, 0.0, 0.0]) - x[halves[0]]).max() < 1e-5


def test_bench_gpus_flag_starts_that_many_ranks():
    """`python bench.py --gpus N` ignored the flag (one rank, "n_gpus": 1).  It now starts N ranks itself
    when no launcher did (the driver's `python -m torch.distributed.run --nproc-per-node N` line), and a mismatch between
    --gpus and WORLD_SIZE is an error.  Without GPUs every rank fails loudly: the hot path has no CPU fallback."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if pkg.device_count() > 0:
        pytest.skip("CPU-only check of the launcher")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode != 0
    # two ranks were started (announced before the heavy imports: the launcher kills the other ranks as soon as one has failed, so only
    # the first rank to get there is sure to print why) and the one that got furthest refused to run without its device
    assert "rank 0 of 2 started" in out and "rank 1 of 2 started" in out, out[-2000:]
    assert "needs HIP device" in out, out[-2000:]
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "4", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode != 0 and "--gpus 4 but WORLD_SIZE=2" in (r.stdout + r.stderr)


# ---------------------------------------------------------------------------------------------------------------------------------
# DISTRIBUTED global solve of ONE body (ADMM_HIP_DIST_SOLVE=1; SURVEY 8e option B, BASELINE configs[3]'s "all-reduce per CG
# iteration"): vertex rows of the PCG split over the ranks, partial dot products + the preconditioned residual summed per iteration.
def _dist_solve_worker(rank, world, port, kind, n, frames, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ["ADMM_HIP_DIST_SOLVE"] = "1"
    os.environ["ADMM_HIP_UZ_FREEZE"] = "1"        # (contact: active set fixed per step, as in test_step_uzawa_frozen_active_set_is_tight)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sc = _dist_scene(kind, n)
    soft = _DIST_SOFT.get(kind, 0)
    s = sc.make_solver(device=0, pcg_tol=1e-10 if soft else 1e-12, pcg_max_iters=2000, rank=rank, world_size=world)
    calls = [0, 0]

    def allreduce(buf):
        calls[0] += 1; calls[1] += buf.size
        dist.all_reduce(torch.from_numpy(buf))
    s.set_rhs_allreduce(allreduce)
    if soft:      # a COLLECTIVE call with the distributed solve: every K^-1 X of the inverse iteration is one distributed solve
        s.compute_soft_modes(soft, 3)      # (three rounds of inverse iteration instead of eight: every K^-1 X travels over gloo here)
        calls[0] = calls[1] = 0
    iters = 0
    for _ in range(frames):
        s.step()
        rd = s.runtime_data()
        assert rd.unconverged_solves == 0
        iters += rd.inner_iters
    q.put((rank, s.m_x.copy(), iters, calls[0], calls[1]))
    s.close()
    dist.destroy_process_group()


_DIST_SOFT = {"soft": 8, "bigsoft": 12}      # kinds that run with the soft-mode Galerkin step (round 6: the distributed solve no longer refuses it)


def _dist_scene(kind, n):
    if kind in ("soft", "bigsoft"):
        kind = "big" if kind == "bigsoft" else "pcg"
    if kind == "big":        # ONE body beyond the chip's LDS (> 262 144 vertices): no on-chip plan on any rank count
        return scenes.blob_scene(n, admm_iters=3, linsolver=0)
    if kind == "floor":      # a cube dropped on a Floor: UzawaCG with an active set, K^-1 columns solved by the distributed PCG
        sc = scenes.mixed_cube_scene(n, admm_iters=8, linsolver=2)
        sc.pins.clear()
        sc.x = sc.x + np.array([0.0, 0.004, 0.0])
        sc.obstacles.append((0, [0.0, 0.0, 0.0, 0.0]))
        return sc
    return scenes.mixed_cube_scene(n, admm_iters=8, linsolver=0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,world", [("pcg", 2), ("pcg", 3), ("floor", 2), ("big", 2), ("big", 8), ("soft", 2), ("bigsoft", 8)])
def test_distributed_solve_matches_single_context(kind, world):
    """Ranks of one body with the PCG's rows split between them (all on device 0, the exchange over gloo through
    admm_hip_set_rhs_allreduce) against the single context at the same tolerance: same iterates up to summation order, every rank
    holds the whole state after every step, and the collectives per solve are the ones DESIGN 6 prices
    (1 per ADMM iteration for b + per solve 2 + 2 per PCG iteration [+1 less on the converged one] + 1 for x)."""
    import multiprocessing as mp          # (stdlib: the pytest process itself never imports torch -- its bundled ROCm libraries next to the system ones the library loads abort at exit)
    n, frames = 9, 3
    soft = _DIST_SOFT.get(kind, 0)      # "soft" / "bigsoft": the same two bodies with the end projection on the softest modes (and the start step in
                                        # front of a frame's second solve), modes computed COLLECTIVELY by the ranks' own distributed solves
    if kind in ("big", "bigsoft"):        # round-4 review item 3: world-2 and world-8 rank contexts of a body that does NOT fit one chip (307 k vertices), the
        n, frames = 140, 1   # launch-path two-level PCG on contiguous ranges of aggregates, interface rows of u exchanged (csrc/pcg_big.hpp)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dist_solve_worker, args=(r, world, port, kind, n, frames, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=600) for _ in range(world))      # (a rank that dies leaves the others in a collective: fail in minutes, not in half an hour)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    sc = _dist_scene(kind, n)
    os.environ["ADMM_HIP_UZ_FREEZE"] = "1"
    try:
        single = sc.make_solver(pcg_tol=1e-10 if soft else 1e-12, pcg_max_iters=2000)
        if soft:
            single.compute_soft_modes(soft, 3)
    finally:
        os.environ.pop("ADMM_HIP_UZ_FREEZE")
    it1 = 0
    for _ in range(frames):
        single.step(); it1 += single.runtime_data().inner_iters
    assert np.abs(single.m_x - sc.x.ravel()).max() > 1e-4
    for rank, x, iters, ncalls, nbytes in got:
        assert scenes.rel_err(x, single.m_x) < (1e-9 if kind == "pcg" else 1e-7), (rank, scenes.rel_err(x, single.m_x))      # (soft kinds: both sides at 1e-10 + modes)
        assert np.array_equal(x, got[0][1])                       # every rank ends with the SAME bits (replicated scalars, summed vectors)
        assert iters == got[0][2] and ncalls == got[0][3]
    if kind in ("big", "bigsoft"):
        assert len(sc.x) > 262144 and single.persistent_launches()["pcg"] == 0
        assert got[0][2] <= it1 + 3 * frames * 3           # the same preconditioner on every rank count: the same iteration counts (+- round-off)
    print("distributed solve (%s, world %d): PCG iterations %d vs single context %d, %d collectives, %.1f MB exchanged per rank" % (kind, world, got[0][2], it1, got[0][3], 8e-6 * got[0][4]))
    single.close()
