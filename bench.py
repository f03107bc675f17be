#!/usr/bin/env python3
"""Headline benchmark: uniform_filter(size=5) on a 512^3 float32 volume.

    python bench.py --gpus N --steps K --warmup W [--config H|E] [--scaling strong|weak] [--dump-outputs DIR] [--full]

Default (--config H, the metric of BASELINE.json).  N = 1: one fused HIP launch per step on a device-resident volume
(cupyimg_amd.scipy.ndimage.uniform_filter -> mi_separable3d_f32).
N > 1 (launched by torch.distributed.run, one rank per GPU): the same 512^3
volume is slab-partitioned on axis 0 (strong scaling); a step is one RCCL halo
exchange of the slab faces plus the fused filter on the rank's extended slab.
torch.distributed (gloo, CPU) is used for the rendezvous, the barriers and the
max-over-ranks reduction only -- all device work goes through libmi355img.

One JSON line is printed by rank 0.  `value` = voxels of the whole volume per
second (Mvoxels/s) with inputs already resident in HBM.  `roofline` prices the
fused kernel against 8.0 TB/s with the ALGORITHMIC 8 B/voxel (SURVEY.md
section 8d), timed live with HIP events on the library's stream.

A plain run does only what `value` needs: set-up (N > 1: the schedule
tuning; N = 1: the W + K steps run once untimed), ~40 ms of copy-kernel load so
that the clocks have settled, the W warm-up and K timed steps, the
--dump-outputs sample, the line.  --full adds everything else, each outside the
timed steps: for N = 1 the figures of that first pass (`cold`) and the
copy-kernel comparators of `roofline` (before the warm-up, in place of the
40 ms of load), `cpu_baseline` -- the CPU oracle (scalar single-thread port)
and scipy.ndimage on the host cores, on the full 512^3 volume, whose outputs
double as a full-size parity check of the GPU result -- and the `configs` block;
for N > 1 the per-rank filter / exchange times and the parity of the slab
result.  `parity_ok` (and exit status 3 on a failure) is reported by --full runs.

--scaling weak: every rank filters its own 512^3 slab of a (512 N) x 512 x 512
volume (per-GPU work fixed).  --config E: BASELINE config 4, uniform_filter
size=9 on a 2048^3 float32 volume slab-split over the N ranks (N = 8: 256 + 8
planes per rank; N = 1: the whole 32 GiB volume on one GPU), generated on the
device by a counter-based generator (csrc/synth.hip) so the volume never exists
on the host; outside the timed region every rank rebuilds the planes around its
two slab faces on the host (oracle/synth.py) and checks seams and outer faces
against scipy.ndimage.
"""
import argparse
import json
import os
import sys
import time

# RCCL between PROCESSES (one rank per GPU) needs dmabuf IPC on this driver: without it the first ncclSend / ncclRecv fails
# with `hipIpcGetMemHandle: invalid argument`.  HSA reads the variable when the runtime initialises (the first HIP call),
# so it is set here, before anything can have touched a device -- never by re-executing the process.  cupyimg_amd._lib.load()
# does the same for every other program that uses the library ("Multi-process launches").
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_SIDE = 512
SIZE = 5
HBM_PEAK_GBS = 8000.0          # MI355X spec (MI355X_MICROARCH.md); best streaming copy measured here: 6450 (copy_bw.hip)
ALG_BYTES_PER_VOXEL = 8        # read 4 + write 4


def synth(shape, seed=0):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)


# --dump-outputs: the whole 512^3 result is 512 MiB, so what is written is a fixed sample of it -- the first and last
# z-plane (where the boundary mode acts) and the voxels at DUMP_SAMPLES seeded flat indices of the whole volume.  The
# indices are global, so a slab-split run writes the same files as a single-GPU run of the same volume.
DUMP_SEED = 20261015
DUMP_SAMPLES = 1 << 22          # 16 MiB of float32; with two 2048^2 planes (config E) 48 MiB in all
DUMP_CHUNK_BYTES = 256 << 20    # device-to-host copies of at most this many bytes at a time


def output_sample(dev, z0, nz):
    """This rank's part of the dump sample of an (nz, Y, X) result whose planes z0 .. z0 + len(dev) are `dev` (device
    array): (sampled values in index order, {z: plane} of the first / last z-plane of the volume held here)."""
    plane = dev.shape[1] * dev.shape[2]
    idx = np.unique(np.random.default_rng(DUMP_SEED).integers(0, nz * plane, DUMP_SAMPLES, dtype=np.int64))
    z1 = z0 + dev.shape[0]
    mine = idx[np.searchsorted(idx, z0 * plane):np.searchsorted(idx, z1 * plane)] - z0 * plane
    vals = np.empty(mine.size, dev.dtype)
    step = max(1, DUMP_CHUNK_BYTES // (plane * dev.dtype.itemsize))
    for a in range(0, dev.shape[0], step):
        b = min(a + step, dev.shape[0])
        s0, s1 = np.searchsorted(mine, [a * plane, b * plane])
        vals[s0:s1] = dev[a:b].get().reshape(-1)[mine[s0:s1] - a * plane]
    faces = {z: dev[z - z0].get() for z in (0, nz - 1) if z0 <= z < z1}
    return vals, faces


def write_dump(directory, parts, name):
    """Merges the ranks' `output_sample` parts (in rank order) and writes DIR/<name>_sample.npy (1-D) and
    DIR/<name>_faces.npy (2, Y, X), in the result's dtype (float32)."""
    os.makedirs(directory, exist_ok=True)
    faces = {}
    for _, f in parts:
        faces.update(f)
    np.save(os.path.join(directory, name + "_sample.npy"), np.concatenate([v for v, _ in parts]))
    np.save(os.path.join(directory, name + "_faces.npy"), np.stack([faces[z] for z in sorted(faces)]))


SETTLE_LAUNCHES = 220        # ~ 40 ms of the 2 x 512 MiB copy kernel before the comparators are timed
TRAFFIC_FILES = ("r6_traffic.json", "r5_traffic.json")


def kernel_signature(name):
    """("sep3d_long3_kernel", ["5", "true"]) from either spelling of a kernel: rocprofv3's demangled
    `void mi::sep3d_long3_kernel<5, true, false, 0, 5>(float const*, ...)` or the library's own
    `mi::sep3d_long3_kernel<5,true> grid=256 (...)` (mi_debug_last_kernel)."""
    import re
    m = re.search(r"([A-Za-z_][A-Za-z_0-9]*)\s*(?:<([^>]*)>)?", name.replace("void ", "").replace("mi::", ""))
    if not m:
        return None, []
    targs = [a.strip() for a in (m.group(2) or "").split(",") if a.strip()]
    return m.group(1), targs


def same_kernel(a, b):
    """True when the two names are the same kernel template and the shorter template-argument list is a prefix of the
    longer one (the library prints the arguments that select the instantiation, rocprofv3 all of them)."""
    (na, ta), (nb, tb) = kernel_signature(a), kernel_signature(b)
    n = min(len(ta), len(tb))
    return na is not None and na == nb and ta[:n] == tb[:n]


def measured_traffic(world, config, kernel_name):
    """(HBM bytes per launch, source) from the rocprofv3 PMC passes of this same command (profiles/r*_traffic.json:
    2 x FETCH_SIZE + WRITE_SIZE, gfx950 correction applied).  Counters cannot be read from inside the process, so this
    is the committed measurement -- labelled as such in the JSON line -- valid for the single-GPU headline workload.
    REFUSED (traffic null, the reason in the source field) when the kernel the counters were collected on is not the
    kernel this run dispatched (mi_debug_last_kernel()): a committed constant must not outlive its kernel."""
    if world != 1 or config != "H":
        return None, None
    for name in TRAFFIC_FILES:
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                rec = json.load(f)
            if not same_kernel(rec.get("kernel", ""), kernel_name):
                return None, ("refused: profiles/{} was collected on `{}`, this run dispatched `{}` -- re-run scripts/profile_bench.sh"
                              .format(name, rec.get("kernel"), kernel_name[:80]))
            return rec["hbm_bytes_per_launch"], "profiles/{} (rocprofv3 PMC passes of this command, not live; kernel name checked against this run's)".format(name)
        except (OSError, KeyError, ValueError):
            continue
    return None, None


def last_kernel():
    """Name of the kernel the last separable-filter call of this thread dispatched, from the library itself."""
    import ctypes
    from cupyimg_amd import _lib
    buf = ctypes.create_string_buffer(200)
    fn = _lib.load().mi_debug_last_kernel
    fn.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    fn(buf, 200)
    return buf.value.decode()


def copy_kernel_ceiling(ca, xd, out):
    """The in-tree float4 copy kernels on the same 2 x 512 MiB, best grid size each: the practical HBM ceiling of THIS
    box for the same byte count.  Returns ((GB/s, blocks) of the r4 copy -- four 16-byte loads in flight per thread,
    loads and stores non-temporal, scripts/diag/copy_bw.hip -- and (GB/s, blocks) of the plain grid-stride copy the
    earlier rounds priced against; hipMemcpy is a weaker comparator than either)."""
    import ctypes
    from cupyimg_amd import _lib
    res = []
    for name, grids in (("mi_debug_copy_f32_nt", (2048, 4096, 8192, 16384)), ("mi_debug_copy_f32", (1024, 2048, 4096, 8192, 16384))):
        fn = getattr(_lib.load(), name)
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
        best, best_blocks = None, None
        # the clocks of a box settle after ~ 40 ms of load (profiles/r3_clock_settle.txt): the ceiling is a settled figure
        if not res:
            for _ in range(SETTLE_LAUNCHES):
                fn(xd.ptr, out.ptr, xd.size, grids[0], None)
        for blocks in grids:
            for _ in range(3):
                fn(xd.ptr, out.ptr, xd.size, blocks, None)
            e0, e1 = ca.Event(), ca.Event()
            e0.record()
            for _ in range(20):
                fn(xd.ptr, out.ptr, xd.size, blocks, None)
            e1.record()
            ca.synchronize()
            t = e0.elapsed_ms(e1) / 20 / 1e3
            if best is None or t < best:
                best, best_blocks = t, blocks
        res.append((2 * xd.nbytes / best / 1e9, best_blocks))
    return res


def settle_device(ca, ms=40.0):
    """~ `ms` of copy-kernel load on two scratch buffers.  The single-GPU headline path times its comparators before
    the warm-up steps (~ 60 ms of load); the slab / multi-rank paths have no comparators, so every rank runs this
    instead -- the same device state before the W warm-up steps for every N, otherwise the N = 1 line would be taken
    with settled clocks and the N > 1 lines inside the slower first 30 ms of a process (profiles/r3_clock_settle.txt)."""
    import ctypes
    from cupyimg_amd import _lib
    fn = _lib.load().mi_debug_copy_f32
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    a = ca.empty((1 << 25,), np.float32)
    b = ca.empty((1 << 25,), np.float32)
    a.fill(0.0)
    e0, e1 = ca.Event(), ca.Event()
    e0.record()
    while True:
        for _ in range(40):
            fn(a.ptr, b.ptr, a.size, 2048, None)
        e1.record()
        ca.synchronize()
        if e0.elapsed_ms(e1) >= ms:
            break
    del a, b


def _allcores_worker(args):
    """One slab of the slab-parallel SciPy run (child process of the CPU-only helper)."""
    name_in, name_out, shape, z0, z1, lo, hi = args
    from multiprocessing import shared_memory
    import scipy.ndimage as sndi
    a = shared_memory.SharedMemory(name=name_in)
    b = shared_memory.SharedMemory(name=name_out)
    x = np.ndarray(shape, np.float32, buffer=a.buf)
    y = np.ndarray(shape, np.float32, buffer=b.buf)
    e0, e1 = max(z0 - lo, 0), min(z1 + hi, shape[0])
    # at a global edge the slab edge is the volume edge, so `reflect` is evaluated exactly as unsplit
    y[z0:z1] = sndi.uniform_filter(x[e0:e1], size=SIZE)[z0 - e0:z0 - e0 + (z1 - z0)]
    a.close()
    b.close()
    return 0


def allcores_helper(nproc):
    """CPU-only helper (run as a child process, never touches the GPU):
    scipy.ndimage.uniform_filter on the same 512^3 volume, z-slabs over `nproc`
    processes sharing memory.  Prints one JSON line."""
    import multiprocessing as mp
    from multiprocessing import shared_memory
    x0 = synth((N_SIDE,) * 3)
    a = shared_memory.SharedMemory(create=True, size=x0.nbytes)
    b = shared_memory.SharedMemory(create=True, size=x0.nbytes)
    try:
        x = np.ndarray(x0.shape, np.float32, buffer=a.buf)
        x[...] = x0
        bounds = np.linspace(0, N_SIDE, nproc + 1).astype(int)
        jobs = [(a.name, b.name, x0.shape, int(bounds[i]), int(bounds[i + 1]), SIZE // 2, SIZE // 2)
                for i in range(nproc) if bounds[i + 1] > bounds[i]]
        best = None
        with mp.get_context("fork").Pool(nproc) as pool:
            pool.map(_allcores_worker, jobs)                       # warm-up (page faults, imports)
            for _ in range(2):
                t0 = time.perf_counter()
                pool.map(_allcores_worker, jobs)
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
        print(json.dumps({"value": round(x0.size / best / 1e6, 1), "unit": "Mvoxels/s", "cores": nproc,
                          "note": "scipy.ndimage.uniform_filter on z-slabs (+2 halo planes) in %d processes, "
                                  "shared memory, best of 2" % nproc}))
    finally:
        a.close(); a.unlink(); b.close(); b.unlink()


def cpu_baseline(x, gpu_out):
    """Oracle (kind "port", 1 core) + scipy.ndimage on the same array."""
    from oracle import ndimage as orc
    orc.build()
    best = None
    ref = None
    for _ in range(2):
        t0 = time.perf_counter()
        ref = orc.uniform3d_f32(x, SIZE, "reflect")
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    res = {
        "value": round(x.size / best / 1e6, 2), "unit": "Mvoxels/s", "cores": 1, "kind": "port",
        "sample": "full 512^3 float32 volume, uniform_filter size=5 reflect, best of 2 "
                  "(oracle/ndimage_oracle.c orc_uniform3d_f32, scalar, single thread)",
        "host_cores_available": os.cpu_count(),
    }
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    res["cpu_model"] = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    try:
        import scipy.ndimage as sndi
        t0 = time.perf_counter()
        sref = sndi.uniform_filter(x, size=SIZE)
        dt = time.perf_counter() - t0
        res["scipy_ndimage"] = {"value": round(x.size / dt / 1e6, 2), "unit": "Mvoxels/s", "cores": 1,
                                "note": "scipy.ndimage.uniform_filter, single-threaded by construction, 1 run"}
        if gpu_out is not None:
            d = np.abs(gpu_out.astype(np.float64) - sref).max()
            res["parity_vs_scipy_maxnorm_rel"] = float(d / np.abs(sref).max())
    except Exception as exc:  # scipy missing on the box
        res["scipy_ndimage"] = {"error": repr(exc)}
    if gpu_out is not None:
        d = np.abs(gpu_out.astype(np.float64) - ref).max()
        res["parity_vs_oracle_maxnorm_rel"] = float(d / np.abs(ref).max())
    # all host cores: SciPy itself is single-threaded, so slabs in separate processes (a child process that
    # never touches the GPU)
    try:
        import subprocess
        nproc = max(1, min(os.cpu_count() or 1, 64))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-allcores-helper", str(nproc)],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=180)
        res["scipy_ndimage_all_cores"] = json.loads(out.stdout.strip().splitlines()[-1])
    except Exception as exc:
        res["scipy_ndimage_all_cores"] = {"error": repr(exc)[:200]}
    return res


# ---------------------------------------------------------------------------------------------------------------------
# The other single-GPU BASELINE.json configs ("plus the four other configs"), timed AFTER the headline's
# timed region and reported in the same JSON line under "configs".  Workloads, inputs and tolerances are those of
# tests/test_gpu_baseline_full.py (tests/helpers/fullsize.py builds them; scipy.ndimage on z sub-slabs over the host
# cores is the comparator: every plane of every output, outside every timed region).
# ---------------------------------------------------------------------------------------------------------------------
CONFIG_MIN_MS = 40.0         # at least this much back-to-back load per timed burst (clocks settle after ~40 ms)


def _time_launches(ca, fn, min_reps=10):
    """Seconds per call: 5 warm launches to size the burst, one untimed burst, one timed burst of >= CONFIG_MIN_MS
    between two HIP events on the library's stream."""
    e0, e1 = ca.Event(), ca.Event()
    e0.record()
    for _ in range(5):
        fn()
    e1.record()
    ca.synchronize()
    per = max(e0.elapsed_ms(e1) / 5, 1e-3)
    reps = max(min_reps, int(CONFIG_MIN_MS / per) + 1)
    for _ in range(reps):
        fn()
    ca.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    ca.synchronize()
    return e0.elapsed_ms(e1) / reps / 1e3, reps


def other_configs(ca, ndi, x_host, xd, out, parity=True):
    """{"B": {...}, "C": ..., "D": ..., "Dprime": ..., "E_slab": ...}: ms per launch (HIP events), fraction of 8 TB/s on
    the ALGORITHMIC bytes, the kernel the library dispatched, and whole-volume parity against scipy.ndimage.  Returns
    (table, all_parity_ok).  `xd` / `out` are the headline's 512^3 buffers (same N(0,1) seed-0 volume); they are dropped
    before the two large configs are staged."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import scipy.ndimage as sndi
    from helpers import fullsize as fs
    table, ok = {}, True

    def entry(name, workload, voxels, bpv, secs, reps, kernel, par_key, par_val, tol):
        nonlocal ok
        gbs = voxels * bpv / secs / 1e9
        e = {"workload": workload, "ms": round(secs * 1e3, 4), "launches_timed": reps, "Mvoxels_per_s": round(voxels / secs / 1e6, 1),
             "alg_bytes_per_voxel": bpv, "achieved_GBps": round(gbs, 1), "frac_of_8TBps": round(gbs / HBM_PEAK_GBS, 4),
             "kernel": kernel[:110]}
        if par_key is not None:
            good = bool(par_val <= tol)
            e["parity"] = {par_key: par_val, "tol": tol, "planes": "all", "ok": good}
            ok = ok and good
        table[name] = e

    n = N_SIDE
    t, reps = _time_launches(ca, lambda: ndi.gaussian_filter(xd, sigma=2, output=out))
    k = ca.last_kernel()
    err = fs.whole_volume_filter(x_host, out.get(), 8, 8, lambda s: sndi.gaussian_filter(s.astype(np.float64), sigma=2),
                                 planes=16) if parity else None
    entry("B", "gaussian_filter sigma=2 (17 taps/axis) on 512^3 float32", n ** 3, 8, t, reps, k,
          "maxnorm_rel_vs_scipy" if parity else None, err, 1e-6)

    M, off = fs.affine_case(n)
    t, reps = _time_launches(ca, lambda: ndi.affine_transform(xd, M, off, order=1, mode="constant", output=out))
    k = ca.last_kernel()
    err = fs.whole_volume_affine(x_host, M, off, out.get()) if parity else None
    entry("Dprime", "affine_transform order=1 (the same 3-D warp as a 3x4 matrix) on 512^3 float32", n ** 3, 8, t, reps, k,
          "abs_err_over_max1_vs_scipy" if parity else None, err, 2e-6)

    coords = fs.affine_coords_f32(n)
    cd = ca.asarray(coords)
    t, reps = _time_launches(ca, lambda: ndi.map_coordinates(xd, cd, order=1, mode="constant", output=out))
    k = ca.last_kernel()
    err = fs.whole_volume_map_coordinates(x_host, coords, out.get()) if parity else None
    entry("D", "map_coordinates order=1 3-D affine warp on 512^3 float32 (+1.5 GiB float32 coordinates)", n ** 3, 20, t, reps, k,
          "abs_err_over_max1_vs_scipy" if parity else None, err, 2e-6)
    del cd, coords

    # E-slab: one rank's share of config 4 (2048^3 over 8 GPUs = 256 planes + 4 halo planes either side)
    ca.free_all_blocks()
    shape = fs.E_SLAB
    xe = fs.slab_volume_f32(shape)
    ed = ca.asarray(xe)
    eo = ca.empty(shape, np.float32)
    t, reps = _time_launches(ca, lambda: ndi.uniform_filter(ed, size=9, output=eo), min_reps=8)
    k = ca.last_kernel()
    err = fs.whole_volume_filter(xe, eo.get(), 4, 4, lambda s: sndi.uniform_filter(s.astype(np.float64), size=9),
                                 planes=4) if parity else None
    entry("E_slab", "uniform_filter size=9 on one rank's 264x2048x2048 float32 slab of the 2048^3 volume (config 4 at 8 GPUs)",
          shape[0] * shape[1] * shape[2], 8, t, reps, k, "maxnorm_rel_vs_scipy" if parity else None, err, 1e-6)
    del ed, eo, xe
    ca.free_all_blocks()

    m = fs.N_C
    u = fs.volume_u8((m, m, m), seed=1)
    ud = ca.asarray(u)
    uo = ca.empty(ud.shape, np.uint8)
    t, reps = _time_launches(ca, lambda: ndi.grey_erosion(ud, size=7, output=uo), min_reps=8)
    k = ca.last_kernel()
    bad = fs.whole_volume_filter(u, uo.get(), 3, 3, lambda s: sndi.grey_erosion(s, size=7), exact=True, planes=16) if parity else None
    entry("C", "grey_erosion size=7 on 1024^3 uint8", m ** 3, 2, t, reps, k,
          "voxels_differing_from_scipy" if parity else None, bad, 0)
    del ud, uo, u
    ca.free_all_blocks()
    return table, ok


PIPE_NBUF = 3                # resident input slabs of the pipelined schedule (scripts/bench_slab_step.py: 3 beats 2)
GRAPH_ROTATIONS = 8          # rotations per hipGraph replay of the pipelined_graph candidate
TUNE_BURST = 30              # steps per burst when the schedules are timed

E_SIDE = 2048
E_SIZE = 9
E_SEED = 20260


def quiet_c_stdout(fn):
    """Run fn() with the C-level stdout (fd 1) pointed at stderr: RCCL prints a version banner to stdout when a
    communicator is created, and the one JSON line is the only thing this program may write there."""
    import ctypes
    sys.stdout.flush()
    libc = ctypes.CDLL(None)
    saved = os.dup(1)
    os.dup2(2, 1)
    try:
        return fn()
    finally:
        libc.fflush(None)
        os.dup2(saved, 1)
        os.close(saved)


def fill_synthetic(ca, dst, first_index, seed):
    """dst (C-contiguous float32 device array) <- synthetic values of global indices first_index .. (csrc/synth.hip)"""
    import ctypes
    from cupyimg_amd import _lib
    fn = _lib.load().mi_debug_fill_synthetic_f32
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
    _lib.check(fn(dst.ptr, dst.size, int(first_index), int(seed), None))


def e_seam_parity(plan, local_out, nz, plane_shape, size, seed):
    """Config E, outside the timed region: this rank's first and last 6 output planes (the planes whose taps cross a
    slab seam, or the outer faces of the volume on the edge ranks) against scipy.ndimage on host planes rebuilt from
    the same counter-based generator.  Returns the worst max-norm relative error."""
    import scipy.ndimage as sndi
    from oracle import synth as osynth
    r = size // 2
    worst = 0.0
    for a, b in ((plan.z0, min(plan.z0 + 6, plan.z1)), (max(plan.z1 - 6, plan.z0), plan.z1)):
        e0, e1 = max(a - r, 0), min(b + r, nz)              # at a global edge the block edge is the volume edge
        host = osynth.synthetic_planes(e0, e1, plane_shape, seed)
        ref = sndi.uniform_filter(host.astype(np.float64), size=size)[a - e0:a - e0 + (b - a)]
        got = local_out[a - plan.z0:b - plan.z0].get().astype(np.float64)
        worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", choices=["H", "E"], default="H",
                    help="H: uniform_filter 5 on 512^3 (BASELINE metric, default); E: uniform_filter 9 on 2048^3 slab-split")
    ap.add_argument("--scaling", choices=["strong", "weak"], default="strong",
                    help="config H with N > 1: the 512^3 volume split over the ranks (strong, default) or one 512^3 slab "
                         "per rank (weak)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline, measure and check everything else: cold run, copy-kernel comparators, CPU "
                         "baseline, whole-volume parity and the `configs` block (N = 1); per-rank times and slab parity (N > 1)")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the CPU baseline leg")
    ap.add_argument("--no-configs", action="store_true",
                    help="--full, N = 1, config H: skip the `configs` block (BASELINE configs B, C, D, D', E-slab timed after the headline)")
    ap.add_argument("--schedule", choices=["auto", "plain", "overlapped", "pipelined", "pipelined_graph"], default="auto",
                    help="N > 1 (and --self-loop): schedule of a step (exchange + filter).  auto (default): every candidate is "
                         "timed in bursts of back-to-back steps inside the untimed set-up, the slowest rank's figure decides, "
                         "all ranks take the same one")
    ap.add_argument("--self-loop", action="store_true",
                    help="functional dry run of the N > 1 code path on ONE GPU: the rank is both neighbours of itself (closed chain, "
                         "`wrap` along z) over a one-rank RCCL communicator -- exchange, schedule tuning, seam parity all execute; "
                         "the number it prints is not a benchmark result")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write a fixed seeded sample of what the last step computed to "
                         "DIR/uniform_filter_sample.npy and DIR/uniform_filter_faces.npy (float32), for comparing builds")
    ap.add_argument("--cpu-allcores-helper", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")
    if args.cpu_allcores_helper:
        allcores_helper(args.cpu_allcores_helper)
        return

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit("--gpus {} needs torch.distributed.run with {} ranks (WORLD_SIZE={})".format(
            args.gpus, args.gpus, world))

    import cupyimg_amd as ca
    from cupyimg_amd import distributed as dist_
    from cupyimg_amd.scipy import ndimage as ndi

    if not ca.is_available():
        raise SystemExit("bench.py needs an MI355X; no HIP device is visible")
    # one rank per GPU.  RCCL refuses a communicator with two ranks on one device ("Duplicate GPU detected",
    # ncclInvalidUsage), so fewer GPUs than ranks is an error here, not a dry run (the one-GPU dry run is --self-loop)
    if world > 1 and ca.device_count() < world:
        raise SystemExit("bench.py --gpus {}: {} ranks need {} GPUs, this box shows {} (RCCL does not accept two ranks "
                         "on one device; use --self-loop for a one-GPU dry run of the exchange path)".format(
                             args.gpus, world, world, ca.device_count()))
    ca.set_device(local_rank)

    dist = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)

    def barrier():
        ca.synchronize()
        if dist is not None:
            dist.barrier()

    def exchange_id(uid):
        box = [uid]
        dist.broadcast_object_list(box, src=0)
        return box[0]

    # ------------------------------------------------------------ workload
    cfg = args.config
    weak = cfg == "H" and args.scaling == "weak" and world > 1
    size = SIZE if cfg == "H" else E_SIZE
    side = N_SIDE if cfg == "H" else E_SIDE
    nz_total = side * world if weak else side
    plane_shape = (side, side)
    sf = plan = pipe = rank_us = None
    schedule, sched_ms = "single GPU", {}
    x_host = xd = out = None
    if cfg == "H" and world == 1 and not args.self_loop:
        x_host = synth((N_SIDE,) * 3)
        xd = ca.asarray(x_host)
        out = ca.empty(xd.shape, np.float32)

        def run_steps(n):
            for _ in range(n):
                ndi.uniform_filter(xd, size=SIZE, output=out)
    else:
        lo, hi = dist_.halo_widths(size)
        if args.self_loop:
            plan = dist_.SlabPlan.self_loop(nz_total, lo, hi)
            comm = quiet_c_stdout(lambda: dist_.HaloComm(1, 0, lambda uid: uid))
        else:
            plan = dist_.SlabPlan(nz_total, world, rank, lo, hi, wrap=False)
            comm = quiet_c_stdout(lambda: dist_.HaloComm(world, rank, exchange_id)) if world > 1 else None
        def reduce_max(vals):
            if dist is None:
                return list(vals)
            import torch
            t = torch.tensor(list(vals), dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return [float(v) for v in t]

        sf = dist_.SlabFilter(plan, plane_shape, np.float32, comm, reduce_max=reduce_max)
        sf.autotune = False
        if cfg == "H" and not weak:
            x_host = synth((N_SIDE,) * 3)
            sf.local_in[...] = ca.asarray(x_host[plan.z0:plan.z1])
        else:
            # per-rank generation on the device, keyed by the GLOBAL linear index: no rank ever holds the volume
            fill_synthetic(ca, sf.local_in, plan.z0 * side * side, E_SEED)
        # The pipelined schedule filters a SEQUENCE of resident input slabs (here: three copies of the rank's slab), the
        # halo exchange of the next one underneath the single launch of the current one; plain / overlapped exchange and
        # filter the same slab inside every step.  All of them do one RCCL exchange and one full filter per step.
        has_comm = comm is not None
        pipe = sf.uniform_pipeline(size, nbuf=PIPE_NBUF) if has_comm else None
        if pipe is not None:
            for k in range(1, pipe.nbuf):
                pipe.inputs[k][...] = sf.ext_in
        runners = {"plain": lambda n: [sf.uniform_filter(size, overlap=False) for _ in range(n)]}
        if has_comm:
            runners["overlapped"] = lambda n: [sf.uniform_filter(size, overlap=True) for _ in range(n)]
            runners["pipelined"] = lambda n: pipe.run(n, 0)
            # hipGraph replay of the pipelined rotation: only on request (--schedule pipelined_graph) or in the self-loop
            # dry run -- it measured no faster than direct queuing on one GPU, and a capture of RCCL send / recv between
            # REAL ranks has never run on this pool: not something to find out inside the driver's scaling run
            if args.self_loop or args.schedule == "pipelined_graph":
                runners["pipelined_graph"] = lambda n: pipe.run(n, GRAPH_ROTATIONS * pipe.nbuf)
        sched_ms = {}
        if args.schedule == "auto" and has_comm:
            # burst-timed candidates (what the timed loop below issues: steps back to back, one sync per burst), every
            # rank runs every candidate in the same order (each step is one exchange: the ranks stay paired); medians
            # are maximised over the ranks, so the choice is the same everywhere and suits the slowest rank
            settle_device(ca)
            e0, e1 = ca.Event(), ca.Event()
            for name, fn in runners.items():
                fn(TUNE_BURST)
                ts = []
                for _ in range(3):
                    ca.synchronize()
                    if dist is not None:
                        dist.barrier()
                    e0.record()
                    fn(TUNE_BURST)
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_ms(e1) / TUNE_BURST)
                sched_ms[name] = float(np.median(ts))
            names = list(sched_ms)
            agreed = reduce_max([sched_ms[n] for n in names])
            sched_ms = {n: round(v, 5) for n, v in zip(names, agreed)}
            schedule = min(names, key=lambda n: sched_ms[n])
        else:
            schedule = args.schedule if (args.schedule != "auto" and has_comm) else "plain"
        run_steps = runners[schedule]
        run_steps(pipe.nbuf * 2 if pipe is not None else 1)
        ca.synchronize()
        # per-rank cost of the two halves of a step, measured alone (HIP events on the launch stream)
        rank_us = None
        if pipe is not None and args.full:
            k_us, ex_us = pipe.measure()
            rank_us = [round(k_us, 2), round(ex_us, 2)]

    def timed_region():
        """W untimed warm-up steps, then exactly K steps between barrier + device synchronisation on both sides.
        Returns (wall seconds, HIP-event milliseconds on the launch stream) of the K steps."""
        run_steps(args.warmup)
        barrier()
        ev0, ev1 = ca.Event(), ca.Event()
        t0 = time.perf_counter()
        ev0.record()
        run_steps(args.steps)
        ev1.record()
        barrier()
        return time.perf_counter() - t0, ev0.elapsed_ms(ev1)

    # `value` is always taken with settled clocks: they settle after ~40 ms of load, at a FASTER state than the one they
    # pass through before (profiles/r3_clock_settle.txt).  The slab / multi-rank paths get ~40 ms of the copy kernel on
    # scratch buffers (after the schedule tuning), one state for every N.  The single-GPU headline first runs the W + K
    # steps once (COLD: the first work of the process after the upload), then the same W + K steps again once the clocks
    # have settled (SETTLED, `value`).  Between the two, a --full run measures the comparators of
    # the roofline block (in-tree float4 copy kernel, hipMemcpy D2D; ~60 ms of load on the same buffers), i.e. the filter
    # and its ceilings in the same state, and prints the cold run beside `value` (`cold`); a plain run settles with the
    # ~40 ms of copy kernel instead.  The cold pass stays in a plain run: without it the settled steps measured 1-2 %
    # slower on average, with it they match a --full run.
    comparators = None
    cold = None
    if rank == 0 and cfg == "H" and world == 1 and not args.self_loop:
        cold = timed_region()
        if args.full:
            (ck_gbs, ck_blocks), (ck_plain_gbs, ck_plain_blocks) = copy_kernel_ceiling(ca, xd, out)
            for _ in range(3):
                out[...] = xd
            c0, c1 = ca.Event(), ca.Event()
            c0.record()
            for _ in range(10):
                out[...] = xd
            c1.record()
            ca.synchronize()
            comparators = (ck_gbs, ck_blocks, ALG_BYTES_PER_VOXEL * (N_SIDE ** 3) / (c0.elapsed_ms(c1) / 10 / 1e3) / 1e9,
                           ck_plain_gbs, ck_plain_blocks)
        else:
            settle_device(ca)
    else:
        settle_device(ca)
    elapsed, dev_ms = timed_region()
    kernel_name = last_kernel()
    if args.dump_outputs:
        # read before anything else runs: the configs block below reuses `out`
        part = output_sample(out, 0, nz_total) if sf is None else output_sample(sf.local_out, plan.z0, nz_total)
        parts = [part]
        if dist is not None:
            parts = [None] * world if rank == 0 else None
            dist.gather_object(part, parts, dst=0)
        if rank == 0:
            write_dump(args.dump_outputs, parts, "uniform_filter")
        del part, parts

    # ------------------------------------------------------------ parity of the distributed / slab result (untimed)
    slab_ok = seam_err = None
    if sf is not None and args.full:
        if args.self_loop:
            # closed chain of one rank: the halos are the periodic continuation, i.e. `wrap` along z
            full = ndi.uniform_filter(sf.local_in, size=size, mode=["wrap", "reflect", "reflect"])
            slab_ok = not ca.arrays_differ(sf.local_out, full)
            del full
        elif cfg == "H" and not weak:
            # every rank filters the whole volume on its own GPU and checks that its slab of the distributed result
            # is bit-identical to it
            full = ndi.uniform_filter(ca.asarray(x_host), size=SIZE)
            slab_ok = not ca.arrays_differ(sf.local_out, full[plan.z0:plan.z1])
            del full
        else:
            seam_err = e_seam_parity(plan, sf.local_out, nz_total, plane_shape, size, E_SEED)
    rank_table = None
    if dist is not None:
        import torch
        t = torch.tensor([elapsed, dev_ms, 0.0 if slab_ok in (None, True) else 1.0, seam_err or 0.0], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, dev_ms = float(t[0]), float(t[1])
        if slab_ok is not None:
            slab_ok = t[2].item() == 0.0
        if seam_err is not None:
            seam_err = float(t[3])
        if rank_us is not None:
            g = [torch.zeros(2, dtype=torch.float64) for _ in range(world)]
            dist.all_gather(g, torch.tensor(rank_us, dtype=torch.float64))
            rank_table = [[round(float(v[0]), 2), round(float(v[1]), 2)] for v in g]
    elif sf is not None and rank_us is not None:
        rank_table = [rank_us]
    parity_tol = 1e-6
    parity_ok = (slab_ok in (None, True)) and (seam_err is None or seam_err <= parity_tol)

    voxels = nz_total * side * side
    ms_per_step = elapsed / args.steps * 1e3
    value = voxels / (elapsed / args.steps) / 1e6

    if rank == 0:
        kernel_s = dev_ms / 1e3 / args.steps          # HIP-event time per step on the launch stream (max over ranks)
        per_gpu_voxels = voxels / world
        achieved = ALG_BYTES_PER_VOXEL * per_gpu_voxels / kernel_s / 1e9
        traffic, traffic_source = measured_traffic(world, cfg, kernel_name) if not args.self_loop else (None, None)
        roofline = {
            "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_source,
            "kernel": kernel_name, "kernel_source": "mi_debug_last_kernel() after the timed region",
            "alg_bytes_per_launch": ALG_BYTES_PER_VOXEL * per_gpu_voxels,
            "avg_launch_us": round(kernel_s * 1e6, 2),
        }
        if comparators is not None:
            # the practical ceiling of this box for the same 2 x 512 MiB: the in-tree float4 copy kernel (best grid)
            # and, for continuity with earlier rounds, a hipMemcpy device-to-device copy (both measured before the
            # timed region, see above)
            ck_gbs, ck_blocks, copy_gbs, ck_plain_gbs, ck_plain_blocks = comparators
            roofline["copy_kernel_GBps_same_bytes"] = round(ck_gbs, 1)
            roofline["copy_kernel"] = "copy_f4_nt_kernel: 4 x 16-byte loads in flight per thread, non-temporal loads and stores (r4)"
            roofline["copy_kernel_blocks"] = ck_blocks
            roofline["frac_of_copy_kernel"] = round(achieved / ck_gbs, 4)
            roofline["plain_copy_kernel_GBps_same_bytes"] = round(ck_plain_gbs, 1)      # the comparator of rounds 1-3
            roofline["frac_of_plain_copy_kernel"] = round(achieved / ck_plain_gbs, 4)
            roofline["d2d_copy_GBps_same_bytes"] = round(copy_gbs, 1)
            roofline["frac_of_d2d_copy"] = round(achieved / copy_gbs, 4)
            roofline["comparators_measured"] = "before the warm-up steps, on the same buffers, after {} settling launches of the copy kernel (~40 ms)".format(SETTLE_LAUNCHES)
        if args.full and cfg == "H" and world == 1 and not args.no_cpu and not args.self_loop:
            cpu = cpu_baseline(x_host, out.get())
        else:
            cpu = None
        sched_info = None
        if world == 1 and not args.self_loop:
            partition = "single GPU"
        else:
            partition = "z-slabs x{} + RCCL send/recv halo exchange, {} schedule".format(world, schedule)
            if args.self_loop:
                partition = "SELF-LOOP DRY RUN (one GPU is both neighbours of itself; not a benchmark result): " + partition
            sched_info = {
                "chosen": schedule, "how": ("measured: bursts of {} back-to-back steps per candidate, median of 3, max over ranks; same "
                                            "choice on every rank".format(TUNE_BURST) if sched_ms else "given (--schedule) or no neighbours"),
                "candidates_ms_per_step": sched_ms or None,
                "pipelined": ("{} resident input slabs per rank; the halo exchange of the next slab runs on a second stream under "
                              "the single launch that filters the current one; pipelined_graph replays a hipGraph of {} rotations"
                              .format(PIPE_NBUF, GRAPH_ROTATIONS)),
                "pipe_info": pipe.info() if pipe is not None else None,
                "per_rank_us_[filter_launch_alone, rccl_exchange_alone]": rank_table,
            }
        if cfg == "H":
            metric = "Mvoxels/s, uniform_filter size=5 on 512^3 float32"
            workload = ("uniform_filter size=5 mode=reflect on {}x512x512 float32, device resident".format(nz_total))
        else:
            metric = "Mvoxels/s, uniform_filter size=9 on 2048^3 float32 (BASELINE config 4)"
            workload = "uniform_filter size=9 mode=reflect on 2048x2048x2048 float32, counter-based synthetic data generated per rank on the device"
        line = {
            "metric": metric,
            "value": round(value, 1), "unit": "Mvoxels/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
            "scaling": "weak" if weak else "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic", "full": args.full,
            "config": {"workload": workload, "partition": partition, "device": ca.device_name(),
                       "device_load_before_warmup": ("comparators of the roofline block (~60 ms)" if comparators is not None
                                                     else "the W + K steps once, then 40 ms of the in-tree copy kernel on scratch buffers"
                                                     if cold is not None else "40 ms of the in-tree copy kernel on scratch buffers, every rank")},
            "roofline": roofline,
            "cpu_baseline": cpu,
        }
        if cold is not None and args.full:
            c_el, c_dev = cold
            c_ach = ALG_BYTES_PER_VOXEL * per_gpu_voxels / (c_dev / 1e3 / args.steps) / 1e9
            line["value_state"] = ("settled: the W + K steps ran right after the comparators of the roofline block (~60 ms of copy-kernel "
                                   "load on the same buffers); `cold` = the same W + K steps as the first work of the process")
            line["cold"] = {"value": round(voxels / (c_el / args.steps) / 1e6, 1), "ms_per_step": round(c_el / args.steps * 1e3, 4),
                            "roofline_frac": round(c_ach / HBM_PEAK_GBS, 4), "avg_launch_us": round(c_dev / args.steps * 1e3, 2)}
        if sched_info is not None:
            line["schedule"] = sched_info
        if args.full and cfg == "H" and world == 1 and not args.self_loop and not args.no_configs:
            # the headline's buffers are reused for B / D' / D and dropped before E-slab and C are staged
            line["configs"], cfg_ok = other_configs(ca, ndi, x_host, xd, out, parity=not args.no_cpu)
            line["configs_note"] = ("timed after the headline's timed region (which they do not touch): >= {:.0f} ms of back-to-back launches "
                                    "each between two HIP events, after an equal untimed burst; parity = every plane against scipy.ndimage"
                                    .format(CONFIG_MIN_MS))
            parity_ok = parity_ok and cfg_ok
        if cpu is not None:
            # single-GPU line: the output of the LAST timed launch against the oracle (and SciPy) over the whole volume
            errs = [cpu.get(k) for k in ("parity_vs_oracle_maxnorm_rel", "parity_vs_scipy_maxnorm_rel") if cpu.get(k) is not None]
            if errs:
                line["whole_volume_parity_maxnorm_rel"] = max(errs)
                line["parity_tol"] = parity_tol
                parity_ok = parity_ok and max(errs) <= parity_tol
        if args.full:
            line["parity_ok"] = bool(parity_ok)
        if slab_ok is not None:
            line["slabs_bit_identical_to_single_gpu"] = slab_ok
        if seam_err is not None:
            line["seam_and_face_parity_vs_scipy_maxnorm_rel"] = seam_err
            line["parity_tol"] = parity_tol
        if not parity_ok:
            line["invalid"] = "parity check failed: this line is not a benchmark result"
        print(json.dumps(line))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if not parity_ok:
        raise SystemExit(3)


if __name__ == "__main__":
    main()
