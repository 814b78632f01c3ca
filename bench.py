#!/usr/bin/env python3
"""bench.py -- hsbench-style block-mode throughput of the GPU literal scan engine.

Metric (BASELINE.json): GB/s scanned in block mode (+ matches/s), whole job over
N GPUs, inputs resident in HBM when the timed region starts.

A "step" is one pass of the hot path over one batch: every rank scans its own
shard (all blocks of the corpus; filter + confirm + records in delivery order on
the device) and, for N > 1, the match records are all-gathered over RCCL.
hsbench protocol (tools/hsbench/main.cpp:502-528, 720-724, 823-839): corpus
pre-loaded, barrier, K repeats, bytes*K/secs.

Workloads; the headline is the one BASELINE.json quotes its
target on:
  fdr10k    config 3's per-GPU shard: 10 000 snort-like literals, 1 GiB of packets per GPU
  teddy64   config 2: 64 literals len 4-8, 1 GiB synthetic packet corpus       ("also", N = 1)
  class256  config 4: 256 class-heavy patterns -> their distinct classes in passes of 8
            over a 4 GiB line corpus (shufti/truffle semantics)                  ("also", N = 1)
  rose1000  config 5: 1000 literal-prefix + tail patterns through hs_scan_batch: GPU literal
            hits feeding the host-side confirm, 2 GiB of packets                  ("also", N = 1)

One JSON line on stdout (rank 0), kept under ~6 KB so that the driver's record holds all of it: the headline with its
`roofline` and `cpu_baseline`, and under `also` one compact object per extra workload (value, roofline, cpu_baseline, parity).
Everything else -- thread sweeps, per-stage breakdowns, table descriptions -- goes to stderr and to bench_details.json
(beside gpurun_out/ when that exists, else beside this file); `details` in the line names it.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# tools/round_profile.sh writes these from rocprofv3 passes of this same command. $HSGPU_PROFILE_DIR (tools/gpu_check.sh: the
# passes of THIS gpurun call, on this box) wins over the newest committed round under profiles/.
ROUNDS = ("r06", "r05", "r04")
SIMD_COUNT, CLOCK_GHZ = 1024, 2.4  # MI355X: 256 CUs x 4 SIMDs; MI355X_MICROARCH.md


def _profile(kind):
    """-> (absolute path | None, label for the line). kind: pmc_summary.json | kernel_stats.csv | filter_sq.json | profile_meta.json"""
    d = os.environ.get("HSGPU_PROFILE_DIR")
    if d and os.path.exists(os.path.join(d, kind)):
        return os.path.join(d, kind), "this call: " + os.path.relpath(os.path.join(d, kind), ROOT)
    for r in ROUNDS:
        rel = os.path.join("profiles", f"{r}_bench_{kind}" if kind != "filter_sq.json" else f"{r}_filter_sq.json")
        if os.path.exists(os.path.join(ROOT, rel)):
            return os.path.join(ROOT, rel), rel
    return None, None


def profile_corpus_bytes():
    """the bytes per launch the committed passes ran at (profile_meta.json; rounds 1-5 profiled the 1 GiB shard)"""
    path, _ = _profile("profile_meta.json")
    try:
        return int(json.load(open(path))["corpus_bytes"]) if path else 1 << 30
    except (OSError, KeyError, ValueError):
        return 1 << 30


def kernel_ms_trace(kernel_prefix):
    """the kernel's average duration in the rocprofv3 --kernel-trace --stats summary of this same command
    (kernel_stats.csv): what roofline.kernel_ms_avg, measured live with HIP events, has to agree with.
    -> (ms | None, source)"""
    import csv

    path, src = _profile("kernel_stats.csv")
    try:
        best = None
        for r in csv.DictReader(open(path)):
            if kernel_prefix in r["Name"] and (best is None or int(r["Calls"]) > best[0]):
                best = (int(r["Calls"]), float(r["AverageNs"]) / 1e6)
        return (round(best[1], 4), src) if best else (None, None)
    except (OSError, KeyError, ValueError, TypeError):
        return None, None


def issue_bounds(filter_kernel, confirm_prefix="hwlm_confirm_kernel"):
    """The two kernels' own issue bounds from SQ_INSTS_VALU of the committed passes (filter_sq.json): wave instructions x 4 cycles
    over 1 024 SIMDs at 2.4 GHz -- the floor of THIS design, tracked beside the roofline fraction (verdict, round 5).
    -> {"filter_ms", "confirm_ms", "source"} | None"""
    path, src = _profile("filter_sq.json")
    try:
        sq = json.load(open(path))
    except (OSError, ValueError, TypeError):
        return None
    out = {}
    for name, e in sq.items():
        if "SQ_INSTS_VALU" not in e:
            continue
        ms = e["SQ_INSTS_VALU"] * 4 / (SIMD_COUNT * CLOCK_GHZ * 1e9) * 1e3
        if name.startswith(filter_kernel.split("<")[0]) and filter_kernel.replace(" ", "") in name.replace(" ", ""):
            out["filter_ms"] = round(ms, 4)
        elif name.startswith(confirm_prefix):  # (the passes hold other workloads' instantiations too: the headline's is the heaviest)
            out["confirm_ms"] = max(out.get("confirm_ms", 0.0), round(ms, 4))
    if not out:
        return None
    out["source"] = src
    return out


HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak, /opt/skills/guides/MI355X_MICROARCH.md
REC_BYTES = 16
WORKLOAD_DESC = {
    "fdr10k": "10000 snort-like literals (8-byte suffixes)",
    "teddy64": "64 literals len 4-8",
}


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def build_shards(name, shard_bytes, shard_ids):
    """the corpus is made of shards built with seeds 10 + shard; a rank's resident corpus is the
    concatenation of its shards (weak scaling: one shard per rank; strong scaling: 8 / N of the same eight)"""
    lits, parts, offs, base = None, [], [np.zeros(1, dtype=np.uint64)], 0
    for sid in shard_ids:
        lits, c, o = build_workload(name, shard_bytes, sid)
        parts.append(c)
        offs.append(o[1:] + np.uint64(base))
        base += int(c.size)
    return lits, (np.concatenate(parts) if len(parts) > 1 else parts[0]), np.concatenate(offs)


_WORKLOAD_CACHE = {}  # fdr10k shards: the headline (all eight), the shard line and the virtual ranks use the same ones


def build_workload(name, total_bytes, seed_shift):
    key = (name, int(total_bytes), int(seed_shift))
    if key in _WORKLOAD_CACHE:
        return _WORKLOAD_CACHE[key]
    out = _build_workload(name, total_bytes, seed_shift)
    if name == "fdr10k":
        _WORKLOAD_CACHE[key] = out
    return out


def _build_workload(name, total_bytes, seed_shift):
    from hyperscan_amd import corpus as cp

    if name == "teddy64":
        lits = cp.teddy_literals(64, seed=2)
        corpus, off = cp.packet_corpus(total_bytes, lits, seed=3 + seed_shift)
    elif name == "fdr10k":
        lits, _full = cp.snort_like_literals(10000, seed=4)
        corpus, off = cp.packet_corpus(total_bytes, lits, seed=10 + seed_shift)
    elif name.startswith("lits") and name[4:].isdigit():  # tuning: N literals of len 4-8 (stride-2 tables)
        lits = cp.teddy_literals(int(name[4:]), seed=2)
        corpus, off = cp.packet_corpus(total_bytes, lits[:256], seed=3 + seed_shift)
    else:
        raise SystemExit(f"unknown workload {name}")
    return lits, corpus, off


def pmc_traffic(kernel_prefix):
    """HBM bytes per launch of the dominant kernel from the PMC passes of this same command (pmc_summary.json: rocprofv3 --pmc
    FETCH_SIZE and --pmc WRITE_SIZE in separate runs, tools/round_profile.sh). Units are KB; on gfx950 FETCH_SIZE counts a wide
    coalesced read stream at half its bytes (MI355X_MICROARCH.md, HBM section), hence the factor 2 on the read side.
    -> (bytes | None, source)"""
    path, src = _profile("pmc_summary.json")
    if not path:
        return None, None
    try:
        for name, e in json.load(open(path)).items():
            if name.startswith(kernel_prefix):
                return int(e["FETCH_SIZE"]["avg_KB"] * 1024 * 2 + e["WRITE_SIZE"]["avg_KB"] * 1024), src
    except Exception:
        pass
    return None, None


def pmc_traffic_sum(kernel_prefix, launches_per_step):
    """the same for a kernel that runs several times per step (the class passes): the average launch x launches"""
    path, src = _profile("pmc_summary.json")
    if not path:
        return None, None
    try:
        fetch = write = n = 0.0
        for name, e in json.load(open(path)).items():
            if name.startswith(kernel_prefix):
                k = e["FETCH_SIZE"]["n"]
                fetch += e["FETCH_SIZE"]["avg_KB"] * k
                write += e["WRITE_SIZE"]["avg_KB"] * k
                n += k
        if n:
            return int((fetch * 2 + write) / n * 1024 * launches_per_step), src
    except Exception:
        pass
    return None, None


def filter_kernel_name(flags):
    b = lambda bit: "true" if flags & bit else "false"
    if flags & 256:
        return "hwlm_filter_kernel<true, false, false, false, false, true, false, false, true, false>"
    cls = ("true, true, true" if flags & 4 else
           "true, true, false" if flags & 2 and not flags & 128 else "true, false, false")
    return f"hwlm_filter_kernel<{cls}, {b(8)}, {b(16)}, {b(32)}, {b(64)}, false, false, {b(1024)}>"


class GpuJob:
    """One rank's resident state: table, corpus/offsets/records in HBM."""

    def __init__(self, lits, corpus, off, device, sibling=None, cap=None):
        import torch

        import hyperscan_amd as H

        self.torch = torch
        self.H = H
        self.dev = torch.device("cuda", device)
        self.scratch = H.Scratch(device)
        if sibling is not None:  # a second scan context over the SAME table and resident corpus
            self.table, self.total, self.nblocks = sibling.table, sibling.total, sibling.nblocks
            self.d_corpus, self.d_off = sibling.d_corpus, sibling.d_off
        else:
            self.table = H.hwlm_build(lits, int(os.environ.get("HSGPU_BUILD_FLAGS", "0")))  # tuning knob
            self.total = int(corpus.size)
            self.nblocks = int(off.size - 1)
            self.d_corpus = torch.from_numpy(corpus).to(self.dev)
            self.d_off = torch.from_numpy(off.view(np.int64)).to(self.dev)
        self.cap = cap or max(1 << 16, self.total // 512)
        self.scratch.enable_timing(True)
        self.d_out = torch.zeros(self.cap * 4, dtype=torch.int32, device=self.dev)
        self.d_count = torch.zeros(1, dtype=torch.int64, device=self.dev)
        assert self.d_corpus.data_ptr() % 16 == 0

    def launch(self):
        """One batch scan (the library's kernel pipeline) on torch's current stream."""
        from hyperscan_amd import hwlm as hw

        stream = self.torch.cuda.current_stream().cuda_stream
        hw.hwlm_scan_dev(self.table, self.scratch, self.d_corpus.data_ptr(), self.total, self.d_off.data_ptr(),
                         self.nblocks, self.d_out.data_ptr(), self.cap, self.d_count.data_ptr(), 0, stream)

    def count(self):
        return int(self.d_count.item())

    def records(self):
        n = min(self.count(), self.cap)
        return self.d_out[: n * 4].view(n, 4).cpu().numpy().astype(np.uint32)


def host_cpu_desc():
    model = "?"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return model


def cgroup_cpu_quota():
    """CPUs' worth of time this process's cgroup may use (cgroup v2 cpu.max, v1 cpu.cfs_quota_us), or None when
    unlimited / not visible: sched_getaffinity can show every CPU of a box whose quota is a handful."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, p = f.read().split()[:2]
        return (None if q == "max" else round(int(q) / int(p), 2)), "/sys/fs/cgroup/cpu.max"
    except (OSError, ValueError):
        pass
    for d in ("/sys/fs/cgroup/cpu", "/sys/fs/cgroup/cpu,cpuacct"):
        try:
            q = int(open(d + "/cpu.cfs_quota_us").read())
            p = int(open(d + "/cpu.cfs_period_us").read())
            return (None if q <= 0 else round(q / p, 2)), d + "/cpu.cfs_quota_us"
        except (OSError, ValueError):
            continue
    return None, None


def cpu_baseline(lits, corpus, off, want_seconds=14.0, sample_bytes=256 << 20):
    """The reference's own hwlmExec (oracle/_ref, compiled from /root/reference) -- or the C restatement
    when that library is absent -- timed on this box's host cores over a bounded sample of the same
    workload in hsbench's thread model (tools/hsbench/main.cpp:957-963, 990-1030): T native threads
    pinned one per CPU, each looping over its own slice of the blocks; T = 1 and T = every CPU this
    process may use; with the AVX2 build and -- where the host has the flags -- the AVX-512 VBMI build.
    -> (cpu_baseline object, reference records of the first blocks for the parity gate)"""
    from tests import oracle_binding as ob

    k = max(1, int(np.searchsorted(off, min(sample_bytes, int(off[-1])), side="right")) - 1)
    s_off = np.ascontiguousarray(off[: k + 1])
    s_bytes = int(s_off[-1])
    sample = corpus[:s_bytes]
    cpus = len(os.sched_getaffinity(0))
    if not ob.ref_available():  # the restatement, one thread: a port, not the reference
        o = ob.Oracle(lits)
        t0 = time.perf_counter()
        n = o.count_blocks(sample, s_off)
        dt = time.perf_counter() - t0
        return ({"value": round(s_bytes / dt / 1e9, 4), "unit": "GB/s", "cores": 1, "kind": "port",
                 "sample": f"first {s_bytes} bytes / {k} blocks of the same corpus, oracle/hwlm_oracle.c, 1 thread",
                 "matches_in_sample": int(n)}, None)
    runs, best = {}, None
    quota, quota_src = cgroup_cpu_quota()
    # hsbench -T sweep: 1, 2, 4, ... up to every CPU this process may run on (a cgroup quota below that count shows as
    # the point where the curve stops rising; the best run is the baseline, its thread count is `cores`)
    sweep = sorted({t for t in [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, cpus] if t <= cpus})
    per = want_seconds / (len(sweep) * len(ob.ref_variants()))
    engine = None
    for variant in ob.ref_variants():
        ref = ob.Reference(lits, variant=variant)
        engine = engine or ref.info()
        for T in sweep:
            nbytes, secs, matches, passes = ref.bench_threads(sample, s_off, T, per)
            gbs = nbytes / secs / 1e9
            runs[f"{variant}_T{T}"] = {"GBps": round(gbs, 3), "threads": T, "passes_slowest_thread": passes,
                                       "matches_per_pass": matches}
            if best is None or gbs > best[0]:
                best = (gbs, T, variant, matches)
    t1 = max(v["GBps"] for kk, v in runs.items() if v["threads"] == 1)
    return ({"value": round(best[0], 3), "unit": "GB/s", "cores": best[1], "kind": "reference",
             "sample": f"first {s_bytes} bytes / {k} blocks of the same corpus; hwlmExec per block, T pinned pthreads x own "
                       f"slice, ~{per:.1f}s per run, T swept over {sweep}; best of the runs below ({best[2]} build, T = {best[1]})",
             "engine": engine, "cpu": host_cpu_desc(), "cpus_visible": cpus, "cgroup_cpu_quota": quota,
             "cgroup_cpu_quota_source": quota_src,
             "effective_cores_by_scaling": round(best[0] / t1, 1) if t1 > 0 else None,
             "runs": runs, "matches_in_sample": int(best[3])}, None)


def compare_records(g, want, what):
    """g: GPU records [n, 4] (block, end, id, lit) of some block range, want: the reference's (block, end, id) of the same range.
    The sorted (block, end, id) multisets are identical (unit/internal/fdr.cpp:185-188 compares (end, id) lists the same way)
    and the GPU's records arrive in delivery order."""
    key = (g[:, 0].astype(np.uint64) << np.uint64(32)) | g[:, 1].astype(np.uint64)
    assert np.all((key[1:] > key[:-1]) | ((key[1:] == key[:-1]) & (g[1:, 3] > g[:-1, 3]))), f"records not in delivery order ({what})"
    gi = np.lexsort((g[:, 2], g[:, 1], g[:, 0]))
    wi = np.lexsort((want["id"], want["end"], want["block"]))
    ok = (len(g) == len(want) and np.array_equal(g[gi, 0], want["block"][wi]) and np.array_equal(g[gi, 1], want["end"][wi])
          and np.array_equal(g[gi, 2], want["id"][wi]))
    assert ok, f"PARITY FAILURE on {what}: GPU {len(g)} records vs CPU {len(want)}"


def parity_gate(recs, gate, lits):
    """Content-level parity on the first blocks (the bounded form; reference_gate_full is what the bench runs since round 5)."""
    kg, want = gate
    compare_records(recs[recs[:, 0] < kg], want, f"the first {kg} blocks")
    return f"sorted (block,end,id) multisets identical on the first {kg} blocks ({len(want)} matches); delivery order checked"


def reference_gate_full(lits, corpus, off, recs, what):
    """The WHOLE corpus against the reference (round 4's verdict: the gate covered a quarter of the headline GiB and none of the
    8 GiB): the compiled reference's hwlmExec per block over every block (unit/internal/fdr.cpp:185-188 compares full lists;
    hsbench checks the count per repeat, tools/hsbench/main.cpp:778-787), collected on every host thread at once -- ranges of
    blocks balanced by bytes, each range's (block, end, id) multiset compared with the GPU's records of the same blocks, and the
    GPU's delivery order checked across the whole array. Byte offsets beyond 2^32 are ordinary here (the 8 GiB corpus).
    -> prose for the bench line"""
    from concurrent.futures import ThreadPoolExecutor

    from tests import oracle_binding as ob

    t0 = time.perf_counter()
    real = ob.ref_available()
    ref = ob.Reference(lits, variant=ob.ref_variants()[-1]) if real else ob.Oracle(lits)
    nblocks = int(off.size - 1)
    threads = max(1, min(32, len(os.sched_getaffinity(0))))
    parts = max(1, min(nblocks, threads * 4))
    cuts = np.searchsorted(off, np.linspace(0, int(off[-1]), parts + 1)[1:-1].astype(np.uint64), side="left")
    cuts = np.unique(np.concatenate([[0], cuts, [nblocks]]))
    assert np.all(recs[1:, 0] >= recs[:-1, 0]), "records not in block order"
    idx = np.searchsorted(recs[:, 0], cuts, side="left")

    def one(i):
        lo, hi = int(cuts[i]), int(cuts[i + 1])
        g = recs[int(idx[i]):int(idx[i + 1])]
        if real:
            want = ref.collect_blocks(corpus, off[lo:hi + 1], cap=len(g) + 4096)
        else:
            want = ref.collect_blocks(corpus[int(off[lo]):int(off[hi])], off[lo:hi + 1] - off[lo])
        want["block"] += np.uint32(lo)
        compare_records(g, want, f"blocks [{lo}, {hi}) of {what}")
        return len(want)

    with ThreadPoolExecutor(threads) as ex:
        n = sum(ex.map(one, range(len(cuts) - 1)))
    assert n == len(recs)
    src = "the compiled reference's hwlmExec (oracle/_ref)" if real else "oracle/hwlm_oracle.c"
    return (f"ALL {nblocks} blocks / {n} matches / {int(off[-1])} bytes: sorted (block,end,id) multisets identical to {src}, "
            f"delivery order checked ({time.perf_counter() - t0:.1f}s on {threads} threads)")


def gpu_vs_gpu_gate(job):
    """The whole resident corpus, every record: the default pipeline (confirm workers emit their regions in delivery order,
    a gather kernel places them) against the always-correct fused pipeline + record_sort_kernel on a second scratch -- the two share
    the filter's arithmetic and nothing of what follows it. Identical arrays, element for element, or the bench stops."""
    torch = job.torch
    other = GpuJob(None, None, None, torch.cuda.current_device(), sibling=job, cap=4 * job.cap)  # (the fused kernel stages per filter wavefront: a quarter of the regions)
    other.scratch.set_tuning(1)
    job.launch()
    other.launch()
    torch.cuda.synchronize()
    n, n2 = job.count(), other.count()
    assert n == n2 and n <= job.cap, f"PARITY FAILURE: default pipeline {n} records, fused pipeline {n2}"
    same = bool(torch.equal(job.d_out[: n * 4], other.d_out[: n * 4]))
    assert same, "PARITY FAILURE: the default and the fused pipeline deliver different record arrays"
    del other
    torch.cuda.empty_cache()
    return f"all {n} records of the whole {job.total}-byte corpus identical, element for element, to the fused pipeline's (GPU vs GPU)"


def box_info():
    """what this GPU box is, recorded with every line (round 5 met one box on which every process died with a GPU memory fault: the
    next one should be identifiable): the KFD node of the first GPU, driver and firmware versions, the environment that matters"""
    import glob

    import torch

    out = {"env": {k: os.environ[k] for k in ("HSA_XNACK", "HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "HSA_ENABLE_IPC_MODE_LEGACY") if k in os.environ}}
    try:
        p = torch.cuda.get_device_properties(torch.cuda.current_device())
        out["device"] = {"name": p.name, "arch": getattr(p, "gcnArchName", None), "cus": p.multi_processor_count, "mem_GiB": round(p.total_memory / 2**30, 1)}
        out["torch"], out["hip"] = torch.__version__, torch.version.hip
    except Exception:  # noqa: BLE001
        pass
    for node in sorted(glob.glob("/sys/class/kfd/kfd/topology/nodes/*")):
        try:
            props = dict(l.split(None, 1) for l in open(node + "/properties").read().splitlines() if " " in l)
            if int(props.get("simd_count", "0")) > 0:
                out["kfd"] = {"node": os.path.basename(node), "gpu_id": open(node + "/gpu_id").read().strip(),
                              **{k: props[k].strip() for k in ("unique_id", "fw_version", "sdma_fw_version", "gfx_target_version", "device_id", "num_xcc",
                                                               "simd_count", "lds_size_in_kb", "drm_render_minor") if k in props}}
                break
        except (OSError, ValueError):
            continue
    try:
        out["amdgpu_driver"] = open("/sys/module/amdgpu/version").read().strip()
    except OSError:
        pass
    try:
        out["kernel"] = os.uname().release
    except Exception:  # noqa: BLE001
        pass
    return out


def smi_snapshot():
    """sclk / mclk / socket power / temperature as rocm-smi reports them right now (None when it cannot be read)"""
    import subprocess

    try:
        r = subprocess.run(["/opt/rocm/bin/rocm-smi", "--showclocks", "--showpower", "--showtemp", "--json"], stdout=subprocess.PIPE,
                           stderr=subprocess.DEVNULL, text=True, timeout=20)
        card = next(iter(json.loads(r.stdout).values()))
        out = {}
        for k, v in card.items():
            kl = k.lower()
            if "sclk" in kl and "speed" in kl:
                out["sclk"] = v
            elif "mclk" in kl and "speed" in kl:
                out["mclk"] = v
            elif "power" in kl and ("socket" in kl or "average" in kl or "current" in kl) and "power_W" not in out:
                out["power_W"] = v
            elif "temperature" in kl and ("junction" in kl or "hotspot" in kl) and "temp_C" not in out:
                out["temp_C"] = v
        return out or None
    except Exception:  # noqa: BLE001 -- an aid, never a reason to lose the line
        return None


def run_sustained(job, seconds, what):
    """hsbench times 20 repeats of a whole corpus -- seconds for the reference (tools/hsbench/main.cpp:201,502-528); here 20 steps are
    milliseconds, and round 5 saw the filter kernel drift +11 % inside them while the device's clocks settled. The SAME steps back
    to back for `seconds`: ms per step over the first 20, the last 20 and the whole run (HIP events on the launch stream at steps 0,
    20, N - 20, N: three event records in thousands of launches), the filter / confirm-stage means of the last 30 scans from the
    library's own stamps, rocm-smi before and after. The match count of every step equals the first one's (main.cpp:778-787)."""
    torch = job.torch
    for _ in range(3):
        job.launch()
    torch.cuda.synchronize()
    n0 = job.count()
    t0 = time.perf_counter()
    for _ in range(10):
        job.launch()
    torch.cuda.synchronize()
    est = (time.perf_counter() - t0) / 10
    n = int(max(60, min(20000, seconds / est)))
    time.sleep(1.0)  # the device idle: the run starts from wherever the clocks rest
    smi0 = smi_snapshot()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev[0].record()
    for i in range(n):
        if i == 20:
            ev[1].record()
        if i == n - 20:
            ev[2].record()
        job.launch()
    ev[3].record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    smi1 = smi_snapshot()
    assert job.count() == n0, "match count changed during the sustained run"
    first = ev[0].elapsed_time(ev[1]) / 20
    last = ev[2].elapsed_time(ev[3]) / 20
    whole = ev[0].elapsed_time(ev[3]) / n
    f, c = [], []
    for back in range(30):
        fm, cm, _t = job.scratch.timing(back)
        f.append(fm)
        c.append(cm)
    return {"workload": what, "steps": n, "seconds": round(wall, 3),
            "ms_per_step": {"first20": round(first, 4), "last20": round(last, 4), "whole": round(whole, 4)},
            "GBps": {"first20": round(job.total / first / 1e6, 1), "last20": round(job.total / last / 1e6, 1), "whole": round(job.total / whole / 1e6, 1)},
            "last30_filter_ms": round(float(np.mean(f)), 4), "last30_confirm_stage_ms": round(float(np.mean(c)), 4),
            "drift_last_over_first": round(last / first, 4), "smi_before": smi0, "smi_after": smi1}


def run_virtual_ranks(args, n_ranks, lits, shards, keep_rows=False):
    """The N-rank step loop on ONE GPU (verdict, round 5: the N = 8 prediction was pure arithmetic): every virtual rank scans its own
    1 / N shard (its own scratch, record buffer and stream), packs its records (exchange_pack_kernel) and posts the step's transfers
    over the in-process loopback transport (hsgpu_exchange_loopback_id: a Send meeting its Recv = one device copy), as the RCCL
    transport would at N GPUs; compact (exchange_compact_kernel) after the loop. The scans of N ranks run one after the other
    here, so step_ms is N scans + the exchange: what this measures is everything the exchange costs EXCEPT the wire.
    shards: [(corpus, off)] per rank. -> multi_gpu.loopback"""
    import torch

    from hyperscan_amd import dist as hd

    dev = torch.device("cuda", torch.cuda.current_device())
    jobs = [GpuJob(lits, c, o, dev.index) for c, o in shards]
    for j in jobs:
        j.scratch.enable_timing(False)
    streams = [torch.cuda.Stream(device=dev) for _ in range(n_ranks)]
    for j in jobs:
        j.launch()
    torch.cuda.synchronize()
    counts = [j.count() for j in jobs]
    assert all(c <= j.cap for c, j in zip(counts, jobs))
    bases = np.concatenate([[0], np.cumsum([j.nblocks for j in jobs])])[:n_ranks].tolist()
    rows = max(counts) + 1024
    out = {"n_ranks": n_ranks, "records_per_rank": counts, "what": "N virtual ranks on one GPU over the loopback transport: scan of a 1/N shard each, "
           "pack, the step's transfers as device copies, compact after the loop; no wire"}

    def scans_only(k):
        for _ in range(k):
            for r in range(n_ranks):
                with torch.cuda.stream(streams[r]):
                    jobs[r].launch()
        torch.cuda.synchronize()

    scans_only(2)
    t0 = time.perf_counter()
    scans_only(args.steps)
    out["scan_ms"] = round((time.perf_counter() - t0) / args.steps * 1e3, 4)
    for mode, name in ((hd.NativeExchange.ALL_GATHER, "all_gather"), (hd.NativeExchange.TO_ROOT, "to_root")):
        lid = hd.NativeExchange.loopback_id()
        xs = [hd.NativeExchange(None, n_ranks, r, dev, rows, bases[r], mode=mode, id_bytes=lid) for r in range(n_ranks)]
        for x in xs:
            x.set_counts(counts)
        ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n_ranks)] for _ in range(args.steps)]

        def steps(k, timed):
            for i in range(k):
                for r in range(n_ranks):
                    with torch.cuda.stream(streams[r]):
                        jobs[r].launch()
                        if timed:
                            ev[i][r][0].record()
                        xs[r].step(jobs[r].d_out.view(-1, 4), jobs[r].d_count, cap=jobs[r].cap)
                        if timed:
                            ev[i][r][1].record()
            torch.cuda.synchronize()

        steps(2, False)
        t0 = time.perf_counter()
        steps(args.steps, True)
        step_ms = (time.perf_counter() - t0) / args.steps * 1e3
        ex = [[a.elapsed_time(b) for a, b in row] for row in ev]
        # pack alone: a one-rank exchange has nothing to transfer (hsgpu_exchange_step = exchange_pack_kernel + a local hand-over)
        solo = hd.NativeExchange(None, 1, 0, dev, rows, 0, mode=mode)
        pe = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        with torch.cuda.stream(streams[0]):
            for a, b in pe:
                a.record()
                solo.step(jobs[0].d_out.view(-1, 4), jobs[0].d_count, cap=jobs[0].cap)
                b.record()
        torch.cuda.synchronize()
        pack_ms = float(np.median([a.elapsed_time(b) for a, b in pe]))
        solo.close()
        t0 = time.perf_counter()
        got = [x.compact() for x in xs]
        torch.cuda.synchronize()
        compact_ms = (time.perf_counter() - t0) * 1e3 / (n_ranks if mode == hd.NativeExchange.ALL_GATHER else 1)
        rows0, counts0 = got[0]
        assert counts0 == counts and rows0.shape[0] == sum(counts), "loopback exchange lost records"
        blk = rows0[:, 0].to(torch.int64) & 0xFFFFFFFF
        assert bool((blk[1:] >= blk[:-1]).all()), "gathered records are not in global block order"
        if keep_rows:  # (tests: the gathered rows against ONE scan of the whole corpus)
            out.setdefault("_rows", {})[name] = [g[0].cpu().numpy().astype(np.uint32) for g in got]
        per_rank = float(np.mean(ex))  # a rank's pack + its posted copies, on its own stream
        sent, rcvd = xs[0].wire_bytes()
        out[name] = {"step_ms": round(step_ms, 4), "exchange_ms_per_rank": round(per_rank, 4), "pack_ms": round(pack_ms, 4),
                     "collective_ms": round(max(0.0, per_rank - pack_ms), 4), "compact_ms": round(compact_ms, 4),
                     "step_minus_scans_ms": round(step_ms - out["scan_ms"], 4), "bytes_sent_rank0": sent, "bytes_received_rank0": rcvd}
        for x in xs:
            x.close()
    del jobs
    torch.cuda.empty_cache()
    return out


DUMP_MAX_RECORDS = 1 << 20  # --dump-outputs: records.npy (float64) + record_index.npy stay under 40 MiB


def dump_outputs(ddir, recs):
    """--dump-outputs: what the last timed step handed its caller, as .npy files in float64 (exact for the 32-bit fields).
    records.npy: the match records, one row each (block, end, id, lit), in delivery order; above DUMP_MAX_RECORDS a fixed
    seeded sample of them, and record_index.npy says which rows of the step's output they are.
    matches_per_step.npy: the number of records the step produced."""
    recs = np.asarray(recs).astype(np.uint32)
    n = recs.shape[0]
    idx = np.arange(n) if n <= DUMP_MAX_RECORDS else np.sort(np.random.default_rng(0).choice(n, DUMP_MAX_RECORDS, replace=False))
    os.makedirs(ddir, exist_ok=True)
    np.save(os.path.join(ddir, "records.npy"), recs[idx].astype(np.float64))
    np.save(os.path.join(ddir, "record_index.npy"), idx.astype(np.float64))
    np.save(os.path.join(ddir, "matches_per_step.npy"), np.array([n], dtype=np.float64))
    log(f"outputs of the last timed step: {idx.size} of {n} records -> {ddir}")


def run_workload(name, args, rank, world, dist, do_cpu, dump_dir=None):
    import torch

    total = int(args.gib * (1 << 30))
    t0 = time.perf_counter()
    if getattr(args, "shards_override", None) is not None:  # also.fdr10k_8g: all eight shards on one GPU
        shard_ids = args.shards_override
    elif args.scaling == "strong" and name == args.workload:
        # the same n_shards x gib GiB whatever the rank count: rank r takes a contiguous run of the shards
        assert args.shards % world == 0, "--shards must be a multiple of the rank count"
        per = args.shards // world
        shard_ids = list(range(rank * per, (rank + 1) * per))
    else:
        shard_ids = [rank]
    lits, corpus, off = build_shards(name, total, shard_ids)
    log(f"[rank {rank}] {name}: generated {corpus.size} bytes / {off.size - 1} blocks in {time.perf_counter() - t0:.1f}s")
    job = GpuJob(lits, corpus, off, torch.cuda.current_device())
    info = job.table.info()

    # Software pipelining (--pipeline-depth 2, the default for N > 1): step i+1's scan is launched on a
    # second stream (its own scratch and record buffer, same table and resident corpus) while step i's
    # record all-gather runs on the first. Every step still does all of its work. N = 1 runs serial
    # steps, so that the per-kernel figures are those of the kernels alone.
    depth = max(1, min(2, args.pipeline_depth if args.pipeline_depth else (2 if dist is not None else 1)))
    jobs = [job] + [GpuJob(None, None, None, torch.cuda.current_device(), sibling=job) for _ in range(depth - 1)]
    streams = [torch.cuda.Stream(device=job.dev) for _ in range(depth)]

    def run_steps(n, exch=None, ev=None):
        for i in range(n):
            j = i % depth
            with torch.cuda.stream(streams[j]):
                jobs[j].launch()
                if exch is not None:  # the path's one exchange step: RCCL all-gather of the records over xGMI
                    if ev is not None:
                        ev[i][0].record()
                    exch[j].step(jobs[j].d_out.view(-1, 4), jobs[j].d_count)
                    if ev is not None:
                        ev[i][1].record()
        for st in streams:
            st.synchronize()

    run_steps(max(args.warmup, depth))
    torch.cuda.synchronize()
    n_matches = job.count()
    assert n_matches <= job.cap, "record buffer too small"
    assert all(jb.count() == n_matches for jb in jobs)
    whole_gate = gpu_vs_gpu_gate(job) if (dist is None and rank == 0) else None
    if whole_gate:
        run_steps(1)
        torch.cuda.synchronize()

    exch, second, native, exact, skew, kind = None, None, None, False, 1.0, None
    if dist is not None:
        from hyperscan_amd import dist as hd

        # global block indices: shards are contiguous block ranges, rank r's first block = blocks of ranks < r
        nb = torch.tensor([job.nblocks, n_matches], dtype=torch.int64, device=job.dev)
        allnb = torch.empty(world * 2, dtype=torch.int64, device=job.dev)
        dist.all_gather_into_tensor(allnb, nb)
        allnb = allnb.view(world, 2).cpu()
        base = int(allnb[:rank, 0].sum())
        rows = min(job.cap, int(allnb[:, 1].max()) + 1024)  # every rank posts the same fixed size: the largest count (every step scans the same shard) + slack
        # padded all-gather moves world x max(count) rows per rank, the exact form sum(counts): with skewed shards (one
        # flood-dense shard among quiet ones) the padding is most of the traffic -- choose by the skew of the warm-up counts
        cnts = allnb[:, 1].tolist()
        skew = max(cnts) / max(1.0, float(np.mean(cnts)))

        def make_exchange(which):
            """one exchange object per scan in flight, or None when the C ABI's exchange cannot be created on some rank"""
            if which in ("native", "native_all"):
                # the C ABI's exchange (hsgpu_exchange_*: RCCL directly, 12-byte wire records, exactly the rows every rank found in
                # the warm-up -- every step scans the same shard): to every rank (the all-gather BASELINE.json names), or to the
                # root -- the rank whose host would deliver the callbacks. Every rank must have it, or none uses it.
                try:
                    objs = [hd.NativeExchange(dist, world, rank, job.dev, rows, base,
                                              mode=hd.NativeExchange.ALL_GATHER if which == "native_all" else hd.NativeExchange.TO_ROOT)
                            for _ in jobs]
                    for x in objs:
                        x.set_counts(cnts)
                    ok = 1
                except Exception as e:  # noqa: BLE001 -- any failure means the torch.distributed form for everybody
                    log(f"[rank {rank}] native exchange unavailable: {e}")
                    objs, ok = None, 0
                flag = torch.tensor([ok], dtype=torch.int64, device=job.dev)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                return objs if int(flag.item()) == 1 else None
            if which == "exact":
                bases = np.concatenate([[0], np.cumsum(allnb[:, 0].numpy())])[:world].tolist()
                return [hd.ExactExchange(dist, world, rank, job.dev, cnts, bases) for _ in jobs]
            return [hd.RecordExchange(dist, world, rank, job.dev, rows, base) for _ in jobs]

        def check_gathered(objs, which):
            allr, counts = objs[0].compact()
            assert counts[rank] == n_matches
            if which != "native" or rank == 0:
                assert allr.shape[0] == sum(counts)
                assert bool((allr[1:, 0].to(torch.int64) & 0xFFFFFFFF >= allr[:-1, 0].to(torch.int64) & 0xFFFFFFFF).all()), \
                    "gathered records are not in global block order"

        # `value`'s collective is the all-gather north_star names (auto = native_all); the to-root form -- 1/world of the traffic,
        # what a job whose rank 0 delivers the callbacks needs -- is timed right after it over the same steps, beside it
        kind = "native_all" if args.exchange == "auto" else args.exchange
        exch = make_exchange(kind)
        if exch is None:
            assert args.exchange == "auto", f"--exchange {args.exchange}: hsgpu_exchange_create failed on some rank"
            kind = "exact" if skew > 1.5 else "padded"
            exch = make_exchange(kind)
        native = exch if kind in ("native", "native_all") else None
        exact = kind == "exact"
        run_steps(depth, exch)  # untimed: RCCL sets up its rings on first use
        check_gathered(exch, kind)
        if native is not None:
            kind2 = "native" if kind == "native_all" else "native_all"
            second = make_exchange(kind2)
            if second is not None:
                run_steps(depth, second)
                check_gathered(second, kind2)

    # parity gate against the reference over the WHOLE corpus + the CPU baseline
    cpu, ref_parity = None, None
    if do_cpu:
        # records first: on this stack the scans that directly follow a large D2H copy run ~3x
        # slower for tens of ms (measured: 1.9 vs 0.66 ms per scan, host launch time unchanged);
        # the CPU baseline's seconds in between and one untimed scan keep that out of the timed region
        recs = job.records()
        cpu, _ = cpu_baseline(lits, corpus, off)
        ref_parity = cpu["parity"] = reference_gate_full(lits, corpus, off, recs, name)
        del recs
        run_steps(max(1, args.warmup))  # the W untimed warm-up steps again, right in front of the timed region (the device sat idle for the CPU leg's seconds)
        torch.cuda.synchronize()
    elif getattr(args, "reference_gate", False):  # also.fdr10k_8g: no CPU timing leg, but the same whole-corpus gate
        recs = job.records()
        ref_parity = reference_gate_full(lits, corpus, off, recs, name)
        del recs
        run_steps(max(1, args.warmup))
        torch.cuda.synchronize()

    # timed region: barrier + sync on both sides, exactly K steps
    ev = None
    if dist is not None:
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_steps(args.steps, exch, ev)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    dt = time.perf_counter() - t0
    assert all(jb.count() == n_matches for jb in jobs), "match count changed between repeats"  # hsbench main.cpp:778-787
    last_out = None
    if dump_dir and rank == 0:  # the last timed step's records (N > 1: as gathered), kept on the device until the end
        last = (args.steps - 1) % depth
        last_out = exch[last].compact()[0].clone() if exch is not None else jobs[last].d_out[: n_matches * 4].view(n_matches, 4).clone()
    dt_local, second_res = dt, None
    if second is not None:  # the other collective over the same K steps, same protocol (never `value`)
        ev2 = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        dist.barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        run_steps(args.steps, second, ev2)
        torch.cuda.synchronize()
        dist.barrier()
        dt2 = time.perf_counter() - t1
        tt2 = torch.tensor([dt2], dtype=torch.float64, device=job.dev)
        dist.all_reduce(tt2, op=dist.ReduceOp.MAX)
        g2 = [a.elapsed_time(b) for a, b in ev2]
        s2, r2 = second[0].wire_bytes()
        second_res = {"ms_per_step": round(float(tt2.item()) / args.steps * 1e3, 4), "gather_ms_avg_rank0": round(float(np.mean(g2)), 4),
                      "wire_bytes_sent_rank0": s2, "wire_bytes_received_rank0": r2}
    # HIP events the library recorded on the launch stream around its filter kernel during the timed
    # steps (ring of the last 32 scans); read only now, so the timed loop itself never waited on them
    filt_ms, conf_ms, pipe_ms, span_ms = [], [], [], []
    for jb in jobs:
        for back in range(min(args.steps // depth, 30)):
            f, c, t = jb.scratch.timing(back)
            filt_ms.append(f)
            conf_ms.append(c)
            pipe_ms.append(t)
            span_ms.append(jb.scratch.kernel_span(back))
    kern_avg_s = float(np.mean(filt_ms)) / 1e3

    overlapped = None
    if args.overlap_probe and dist is None and depth == 1:
        # for the record (never `value`): the same steps with two scans in flight on two streams (a second scratch over
        # the same table and resident corpus) -- what hsbench's second thread would add; the per-kernel figures above
        # stay those of serial steps
        j2 = [job, GpuJob(None, None, None, torch.cuda.current_device(), sibling=job)]
        st2 = [torch.cuda.Stream(device=job.dev) for _ in range(2)]

        def run2(n):
            for i in range(n):
                with torch.cuda.stream(st2[i & 1]):
                    j2[i & 1].launch()
            for st in st2:
                st.synchronize()

        run2(4)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        run2(args.steps)
        torch.cuda.synchronize()
        dt2 = time.perf_counter() - t1
        assert j2[1].count() == n_matches
        overlapped = {"ms_per_step": round(dt2 / args.steps * 1e3, 4), "GBps": round(job.total * args.steps / dt2 / 1e9, 2),
                      "what": "the same steps, two scans in flight on two streams (second scratch, same table and corpus)"}
        del j2[1]
    if dist is not None:
        tt = torch.tensor([dt], dtype=torch.float64, device=job.dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
        tot = torch.tensor([job.total, n_matches], dtype=torch.int64, device=job.dev)
        dist.all_reduce(tot)
        all_bytes, all_matches = int(tot[0].item()), int(tot[1].item())
        # every rank's own clock around the same K steps: the per-rank rates (hsbench prints one line per scan thread too)
        mine = torch.tensor([dt_local, float(job.total)], dtype=torch.float64, device=job.dev)
        every = torch.empty(world * 2, dtype=torch.float64, device=job.dev)
        dist.all_gather_into_tensor(every, mine)
        every = every.view(world, 2).cpu().numpy()
        per_rank_gbps = [round(float(b * args.steps / t / 1e9), 2) for t, b in every]
    else:
        all_bytes, all_matches = job.total, n_matches

    # algorithmic bytes: 1 B read per corpus byte -- the filter kernel's -- + 16 B written per match record -- the
    # confirm stage's (its workers stage and place the records; the filter writes none). The dominant kernel is priced on its own
    # bytes, the step on all of them.
    alg_bytes = job.total + REC_BYTES * n_matches
    filter_bytes = job.total
    kname = filter_kernel_name(info["flags"])
    # (the rocprofv3 passes ran this command at ONE size: their figures stand beside a run of that size only)
    same_size = abs(job.total - profile_corpus_bytes()) < (1 << 20)
    trace_ms, trace_src = kernel_ms_trace(kname) if same_size else (None, None)
    step_s = dt / args.steps  # (N > 1: per-rank bytes over the max-over-ranks step time)
    traffic, traffic_src = pmc_traffic(kname) if same_size else (None, None)
    kernel_achieved = filter_bytes / kern_avg_s / 1e9
    step_achieved = alg_bytes / step_s / 1e9
    floor = issue_bounds(kname) if same_size else None
    res = {
        "value": round(all_bytes * args.steps / dt / 1e9, 3),
        "ms_per_step": round(dt / args.steps * 1e3, 4),
        "matches_per_s": round(all_matches * args.steps / dt, 1),
        "matches_per_step": all_matches,
        "roofline": {
            # round 6 (verdict): `achieved` / `frac` are the WHOLE step's -- what `value` is made of: filter + confirm stage + gather +
            # gaps, all algorithmic bytes over ms_per_step; the north-star target (0.5) is on this figure. The dominant kernel's own
            # (its bytes = the corpus, over its HIP-event duration) stand beside it as kernel_achieved / kernel_frac.
            "bound": "hbm", "achieved": round(step_achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(step_achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_src,
            "kernel": kname, "kernel_ms_avg": round(kern_avg_s * 1e3, 4),
            "kernel_achieved": round(kernel_achieved, 2), "kernel_frac": round(kernel_achieved / HBM_PEAK_GBS, 4),
            "kernel_ms_best": round(float(np.min(filt_ms)), 4),
            "kernel_ms_trace": trace_ms, "kernel_ms_trace_source": trace_src,
            "algorithmic_bytes_per_launch": filter_bytes,
            "algorithmic_bytes_per_step": alg_bytes,
            "step_achieved": round(step_achieved, 2), "step_frac": round(step_achieved / HBM_PEAK_GBS, 4),
            "record_bytes_per_step": REC_BYTES * n_matches,
            # the kernel's own execution span from the device wall clock (what rocprofv3's kernel
            # trace reports); the HIP-event interval above also contains the dispatch gaps
            "kernel_ms_device_clock_avg": round(float(np.mean(span_ms)), 4),
            "achieved_device_clock": round(filter_bytes / (float(np.mean(span_ms)) / 1e3) / 1e9, 2),
            "confirm_stage_ms_avg": round(float(np.mean(conf_ms)), 4),
            "pipeline_ms_avg": round(float(np.mean(pipe_ms)), 4),
            "pipeline_GBps": round(alg_bytes / (float(np.mean(pipe_ms)) / 1e3) / 1e9, 2),
        },
        "table": info,
        "records": "in delivery order (block, end, lit), sorted on the device inside the step",
    }
    if floor:
        # this design's own floor: the two kernels' vector instructions x 4 cycles over every SIMD (SQ_INSTS_VALU of the committed
        # passes); step / floor says how much of the step is NOT instruction issue
        tot = floor.get("filter_ms", 0) + floor.get("confirm_ms", 0)
        res["roofline"]["issue_bound_ms"] = {**floor, "sum_ms": round(tot, 4), "step_over_issue_floor": round(step_s * 1e3 / tot, 3) if tot else None}
    res["pipeline_depth"] = depth
    if dist is not None:
        wire = 16 + 12 * max(cnts)
        link = 153e9 * 0.8
        res["multi_gpu"] = {"measured": True, "n_gpus": world, "per_rank_GBps": per_rank_gbps, "per_rank_matches": cnts,
                            "step_ms": round(dt / args.steps * 1e3, 4),
                            "predicted": {"to_root_ms": round(wire / link * 1e3, 4), "ring_all_gather_ms": round((world - 1) * wire / link * 1e3, 4),
                                          "point_to_point_all_gather_ms": round(wire / link * 1e3, 4),
                                          "assumes": "153 GB/s x 0.8 per xGMI link; to-root / point-to-point: every peer over its own link"}}
    if whole_gate:
        res["parity_whole_corpus"] = whole_gate
    if ref_parity:
        res["parity_reference"] = ref_parity
    if overlapped:
        res["two_scans_in_flight"] = overlapped
    if dist is not None:
        g = [a.elapsed_time(b) for a, b in ev]
        if native is not None:
            sent, rcvd = exch[0].wire_bytes()
            names = {"native_all": "all_gather", "native": "to_root"}
            res["exchange"] = {"value_uses": names[kind],
                               "collective": ("hsgpu_exchange_step (C ABI, RCCL): grouped ncclSend / ncclRecv of exactly the agreed rows, 12-byte wire "
                                              "records, " + ("every rank to every rank" if kind == "native_all" else "every rank to rank 0")),
                               "count_skew_max_over_mean": round(skew, 3),
                               names[kind]: {"ms_per_step": round(dt / args.steps * 1e3, 4), "gather_ms_avg_rank0": round(float(np.mean(g)), 4),
                                             "gather_ms_max_rank0": round(float(np.max(g)), 4), "wire_bytes_sent_rank0": sent,
                                             "wire_bytes_received_rank0": rcvd}}
            if second_res is not None:
                res["exchange"][names["native" if kind == "native_all" else "native_all"]] = second_res
        else:
            res["exchange"] = {"value_uses": "exact" if exact else "padded",
                               "collective": ("broadcast x world of exactly counts[r] rows (counts agreed before the timed steps)" if exact else
                                              "all_gather_into_tensor x2 (counts, records padded to a fixed size)"),
                               "count_skew_max_over_mean": round(skew, 3),
                               "rows_per_rank": exch[0].rows, "bytes_per_rank_per_step": exch[0].rows * 16 + 16,
                               "gather_ms_avg_rank0": round(float(np.mean(g)), 4), "gather_ms_max_rank0": round(float(np.max(g)), 4)}
    if do_cpu:
        from hyperscan_amd import hwlm as hw

        # (ii) end to end for the resident case, hsbench's definition (engine_hyperscan.cpp:89-97, 132-145): the scan,
        # then the records to the host and through hsgpu_hwlm_replay into a counting callback
        threads = max(1, min(16, len(os.sched_getaffinity(0))))
        stream = torch.cuda.current_stream().cuda_stream
        ts = []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            job.launch()
            n_rec, n_del = hw.hwlm_fetch_replay_count(job.table, job.scratch, job.d_out.data_ptr(), job.cap, job.d_count.data_ptr(),
                                                      threads, stream)
            ts.append(time.perf_counter() - t0)
        assert n_rec == n_matches and n_del == n_matches
        e2e = float(np.median(ts[1:]))
        # the same with one thread and one copy, for the record of what the threads buy
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        job.launch()
        torch.cuda.synchronize()
        t_scan = time.perf_counter() - t0
        recs_h = job.records()
        t_copy = time.perf_counter() - t0
        n1 = hw.hwlm_replay_count(job.table, recs_h)
        t_one = time.perf_counter() - t0
        assert n1 == n_matches
        res["end_to_end_resident"] = {
            "GBps": round(job.total / e2e / 1e9, 2), "ms": round(e2e * 1e3, 3), "replay_threads": threads,
            "matches_delivered": int(n_del),
            "what": "scan + hsgpu_hwlm_fetch_replay: the sorted records to pinned host memory in 4 chunks, the blocks that have "
                    "arrived replayed on the threads (native counting callback, one counter per thread) while the next chunk copies",
            "single_thread": {"ms": round(t_one * 1e3, 3), "scan_ms": round(t_scan * 1e3, 3),
                              "records_to_host_ms": round((t_copy - t_scan) * 1e3, 3), "replay_ms": round((t_one - t_copy) * 1e3, 3),
                              "what": "scan (synchronous) + D2H of the records (pageable) + hsgpu_hwlm_replay_batch on one thread"}}
        # (iii) (never `value`) the same engine fed from HOST memory: hsgpu_hwlm_exec_batch = H2D of the
        # corpus + the pipeline above + D2H of the records, on a bounded sample
        k = int(np.searchsorted(off, min(256 << 20, int(off[-1])), side="right")) - 1
        s_off = np.ascontiguousarray(off[: k + 1])
        sample = np.ascontiguousarray(corpus[: int(s_off[-1])])
        hw.hwlm_exec_batch(job.table, job.scratch, sample, s_off, cap=job.cap)  # warm: buffers sized
        t0 = time.perf_counter()
        recs_h = hw.hwlm_exec_batch(job.table, job.scratch, sample, s_off, cap=job.cap)
        dt_h = time.perf_counter() - t0
        hw.hwlm_exec_batch_pipelined(job.table, job.scratch, sample, s_off)  # warm: the pipeline's buffers sized
        t0 = time.perf_counter()
        recs_p = hw.hwlm_exec_batch_pipelined(job.table, job.scratch, sample, s_off)
        dt_p = time.perf_counter() - t0
        assert recs_p.size == recs_h.size
        res["host_buffers"] = {"GBps": round(sample.size / dt_h / 1e9, 2), "sample_bytes": int(sample.size),
                               "matches": int(recs_h.size),
                               "pipelined_GBps": round(sample.size / dt_p / 1e9, 2),
                               "pipelined": "hsgpu_hwlm_exec_batch_cb: 64 MiB chunks, the copy of chunk i + 1 beside the scan of chunk i, "
                                            "records handed over per chunk",
                               "what": "hsgpu_hwlm_exec_batch from pageable host memory: H2D of the corpus + scan + "
                                       "D2H of the records; PCIe bound, reported for completeness only"}
    if cpu:
        res["cpu_baseline"] = cpu
    if dist is None and depth == 1 and getattr(args, "sustain_seconds", 0) > 0:
        res["sustained"] = run_sustained(job, args.sustain_seconds, f"{name}, {job.total} bytes resident, serial steps")
    if last_out is not None:
        dump_outputs(dump_dir, last_out.cpu().numpy())
        del last_out
    del job, jobs
    torch.cuda.empty_cache()
    return res


# ---- config 4: class accelerators -----------------------------------------------------------

CLASS_POOL = [("[a-z]", range(ord("a"), ord("z") + 1)), ("[A-Z]", range(ord("A"), ord("Z") + 1)),
              ("[0-9]", range(ord("0"), ord("9") + 1)), ("[a-f0-9]", b"0123456789abcdef"),
              ("\\s", b" \t\r\n\x0b\x0c"), ("[^\\x00-\\x7f]", range(128, 256)), ("[aeiou]", b"aeiou"),
              ("[,.;:]", b",.;:"), ("[A-Za-z_]", b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz_"),
              ("[()\\[\\]]", b"()[]"), ("[-_]", b"-_"), ("\\n", b"\n")]


def run_class256(args):
    """256 patterns A_k{m,}B_k+ ([a-z]{3,}\\d+ style) over a line corpus, one block per line: the GPU work item is
    what the reference's accelerators deliver for such patterns -- class membership and the first / last member per
    block, for every distinct class of the set (src/nfa/shufti.c:150-199, src/nfa/truffle.c:118-165)."""
    import torch

    from hyperscan_amd import accel
    from hyperscan_amd import corpus as cp
    from tests import oracle_binding as ob

    rng = np.random.default_rng(5)
    pats, used, pat_abm = [], set(), []
    for k in range(256):
        a, b = rng.choice(len(CLASS_POOL), 2, replace=False)
        m = int(rng.integers(3, 9))
        pats.append(f"{CLASS_POOL[a][0]}{{{m},}}{CLASS_POOL[b][0]}+")
        pat_abm.append((int(a), int(b), m))
        used |= {int(a), int(b)}
    classes = [accel.CharClass(CLASS_POOL[i][1]) for i in sorted(used)]
    names = [CLASS_POOL[i][0] for i in sorted(used)]
    total_gib = args.class_gib
    t0 = time.perf_counter()
    # total_gib GiB of DISTINCT lines: one generator call per GiB, seeds 5, 6, ... (round 3 laid one GiB out four times)
    reps = max(1, int(total_gib))
    parts, offs, at = [], [], 0
    for r_ in range(reps):
        u, uo = cp.line_corpus(int((total_gib / reps) * (1 << 30)), seed=5 + r_)
        parts.append(u)
        offs.append(uo[:-1] + np.uint64(at))
        at += int(u.size)
    unit, uoff = parts[0], np.concatenate([offs[0], [np.uint64(parts[0].size)]]).astype(np.uint64)
    corpus = np.concatenate(parts) if reps > 1 else parts[0]
    off = np.concatenate(offs + [np.array([at], dtype=np.uint64)]).astype(np.uint64)
    del parts, offs
    total, nb = int(corpus.size), int(off.size - 1)
    log(f"class256: {len(classes)} distinct classes of 256 patterns, {total} bytes / {nb} lines in {time.perf_counter() - t0:.1f}s")
    dev = torch.device("cuda", torch.cuda.current_device())
    d_corpus = torch.from_numpy(corpus).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    # the membership bitmaps of ALL the distinct classes in one read of the corpus (up to 16 per call when neither first nor
    # last is asked for: the patterns need the bitmaps alone)
    assert len(classes) <= accel.CLASS_MAX_BITMAPS
    bm_all, _f, _l = accel.class_scan(classes, d_corpus, total, d_off, nb, False, False)
    cls_buf = (bm_all, None, None, torch.zeros(accel.WORK_BYTES, dtype=torch.uint8, device=dev))
    # parity of the bitmaps, membership bit i <=> corpus[i] in class: 1 MiB at the head of EVERY GiB and the corpus' last MiB
    # (round 4 checked the first MiB of four GiB)
    n = 1 << 20
    cpu = None
    bm_at = sorted({min(g << 30, max(0, total - n)) & ~7 for g in range(int(np.ceil(total / (1 << 30))))} | {max(0, total - n) & ~7})
    for lo8 in bm_at:
        hi8 = min(total, lo8 + n) & ~7
        for ci, cls in enumerate(classes):
            want = np.packbits(np.isin(corpus[lo8:hi8], np.array(cls.members(), dtype=np.uint8)), bitorder="little")
            assert np.array_equal(bm_all[ci][lo8 // 8: hi8 // 8].cpu().numpy(), want), f"class bitmap parity at byte {lo8}"
    # the accelerators' own answer (first / last member per block, shufti.h:40-52), 8 classes per pass: timed beside the
    # patterns' path, which does not need it
    fl = accel.class_scan(classes[:8], d_corpus, total, d_off, nb, True, True)
    fl_buf = (fl[0], fl[1], fl[2], torch.zeros(accel.WORK_BYTES, dtype=torch.uint8, device=dev))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        accel.class_scan(classes[:8], d_corpus, total, d_off, nb, True, True, buffers=fl_buf)
    e1.record()
    torch.cuda.synchronize()
    fl_ms = e0.elapsed_time(e1) / 3
    # the 256 patterns A_k{m,}B_k+ themselves: class indices into the bitmaps, in order
    cls_index = {i: k for k, i in enumerate(sorted(used))}
    seqs = [(cls_index[a], cls_index[b], m, 1, k) for k, (a, b, m) in enumerate(pat_abm)]
    bitmaps = [bm_all[ci] for ci in range(len(classes))]
    # content gate ("final (id,to) vs a brute-force regex oracle"): the records of the first lines against
    # a run-length restatement of the patterns (tests/class_seq_model.py, itself pinned to Python's re), every pattern
    from tests import class_seq_model as csm

    # ... on `--class-gate-mib` MiB of lines (0.74 match ends per corpus byte) with the vectorised model: the first MiB of lines
    # of EVERY GiB and the last MiB of the corpus (round 4: the first 4 MiB of 4 GiB), each slice emitted as one byte range
    per = max(1, args.class_gate_mib) << 20
    starts = sorted({min(g << 30, max(0, total - per)) for g in range(int(np.ceil(total / (1 << 30))))} | {max(0, total - per)})
    n_checked, gate_slices = 0, []
    for lo_byte in starts:
        b0 = int(np.searchsorted(off, lo_byte, side="left"))
        b1 = int(np.searchsorted(off, min(total, int(off[b0]) + per), side="right")) - 1
        if b1 <= b0:
            continue
        g_lo, g_hi = int(off[b0]), int(off[b1])
        vm = csm.VecModel(corpus[g_lo:g_hi], off[b0: b1 + 1] - off[b0])
        counts_g, recs_g, n_emit = accel.class_seq_scan(seqs, bitmaps, total, d_off, nb, (g_lo, g_hi), 1 << 24)
        assert n_emit == len(recs_g), "gate slice overflowed its record buffer"
        order = np.lexsort((recs_g[:, 1], recs_g[:, 0], recs_g[:, 3]))
        recs_g = recs_g[order]
        cuts = np.searchsorted(recs_g[:, 3], np.arange(len(seqs) + 1))
        for k, (a, b, m, n_, _id) in enumerate(seqs):
            w = vm.ends(classes[a].members(), classes[b].members(), m, n_)
            g = recs_g[cuts[k]:cuts[k + 1], :2].astype(np.int64)
            g[:, 0] -= b0
            assert np.array_equal(g, w), (f"PARITY FAILURE: pattern {k} {pats[k]}: GPU {len(g)} match ends vs model {len(w)} in blocks "
                                          f"[{b0}, {b1}) (bytes [{g_lo}, {g_hi}))")
            n_checked += len(w)
        gate_slices.append((b0, b1, g_lo, g_hi))
        del vm
    kg, g_hi = sum(b1 - b0 for b0, b1, _l, _h in gate_slices), sum(h - l for _b0, _b1, l, h in gate_slices)
    # ... and additivity over the GiB parts (lines never cross them: one generator call per GiB): the per-pattern counts of the
    # whole scan equal the sum of the counts of every part scanned ALONE (its own class scan, its own offsets)
    whole_counts, _r, _n = accel.class_seq_scan(seqs, bitmaps, total, d_off, nb, (0, 0), 0)
    whole_counts = whole_counts.cpu().numpy().astype(np.int64)
    part_sum, part_at, n_parts = np.zeros(len(seqs), dtype=np.int64), 0, 0
    bounds = [int(np.searchsorted(off, min(total, (g + 1) << 30), side="left")) for g in range(int(np.ceil(total / (1 << 30))))]
    if len(bounds) > 1 and all(int(off[b]) % 16 == 0 for b in bounds[:-1]) and all(int(off[b]) == min(total, (g + 1) << 30) for g, b in enumerate(bounds)):
        b_lo = 0
        for b_hi in bounds:
            lo_b, hi_b = int(off[b_lo]), int(off[b_hi])
            d_sub_off = torch.from_numpy((off[b_lo: b_hi + 1] - off[b_lo]).view(np.int64)).to(dev)
            sub_bm, _f2, _l2 = accel.class_scan(classes, d_corpus[lo_b:hi_b], hi_b - lo_b, d_sub_off, b_hi - b_lo, False, False)
            c_sub, _r, _n = accel.class_seq_scan(seqs, [sub_bm[ci] for ci in range(len(classes))], hi_b - lo_b, d_sub_off, b_hi - b_lo, (0, 0), 0)
            part_sum += c_sub.cpu().numpy().astype(np.int64)
            n_parts += 1
            b_lo = b_hi
            del sub_bm, d_sub_off
        assert np.array_equal(part_sum, whole_counts), "PARITY FAILURE: per-pattern counts of the whole corpus differ from the sum over its GiB parts"
        torch.cuda.empty_cache()
    seq_buf = accel.class_seq_buffers(len(seqs), total, 0, dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(args.steps)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        ev[i][0].record()
        accel.class_scan(classes, d_corpus, total, d_off, nb, False, False, buffers=cls_buf)
        ev[i][1].record()
        accel.class_seq_scan(seqs, bitmaps, total, d_off, nb, (0, 0), 0, buffers=seq_buf)  # counts only: see `matches`
        ev[i][2].record()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ms = float(np.median([a.elapsed_time(b) for a, b, _c in ev]))
    ms_seq = float(np.median([b.elapsed_time(c) for _a, b, c in ev]))
    n_matches = int(seq_buf[1].sum().item())
    # algorithmic bytes: the corpus read ONCE, one bit per byte and class written
    alg = total * (1 + len(classes) / 8)
    traffic, traffic_src = pmc_traffic_sum("class_bitmap16_kernel", 1)
    if traffic is not None and abs(total - (1 << 30)) > (1 << 20):  # the PMC passes run this workload at 1 GiB: a streaming kernel, scaled by size
        traffic, traffic_src = int(traffic * (total / (1 << 30))), traffic_src + " (1 GiB launch, scaled by corpus size)"
    res = {"workload": f"class256: 256 patterns A{{m,}}B+ over {len(classes)} distinct classes {names}: their membership bitmaps in one "
                       f"read of the corpus, then every pattern's match ends from the bitmaps; "
                       f"{total / (1 << 30):g} GiB of distinct lines (seeded per GiB), {nb} blocks",
           "value": round(total * args.steps / dt / 1e9, 2), "unit": "GB/s of corpus (class bitmaps and all 256 patterns)",
           "ms_per_step": round(dt / args.steps * 1e3, 3),
           "matches_per_step": n_matches, "matches_per_s": round(n_matches * args.steps / dt, 1),
           "matches": "counted per pattern on the device over the whole corpus (several per corpus byte: no record buffer holds them); "
                      "16-byte records are emitted for a byte range on request",
           "parity": f"(block, end) of all 256 patterns on {len(gate_slices)} slices ({kg} lines / {g_hi} bytes, {n_checked} match ends: the head of every GiB "
                     f"and the corpus' tail) identical to the run-length model of tests/class_seq_model.py (pinned to Python re in the CPU suite); "
                     f"per-pattern counts of the whole corpus = the sum over its {n_parts} GiB parts scanned alone; class bitmaps against numpy on "
                     f"{len(bm_at)} x 1 MiB (every GiB and the tail)",
           "class_stage": {"ms": round(ms, 3), "GBps_of_corpus": round(total / (ms / 1e3) / 1e9, 1)},
           "sequence_stage": {"ms": round(ms_seq, 3), "GBps_of_corpus": round(total / (ms_seq / 1e3) / 1e9, 1),
                              "kernel": "class_seq_tile_kernel (one lane per 64-byte word, patterns looped in scalar registers; instruction bound)"},
           "first_last_service": {"ms": round(fl_ms, 3), "classes": 8, "GBps_of_corpus": round(total / (fl_ms / 1e3) / 1e9, 1),
                                  "what": "class_tile_fl_kernel: bitmaps + first / last member per block of 8 classes (what shuftiExec / rshuftiExec return)"},
           "roofline": {"bound": "hbm", "achieved": round(alg / (ms / 1e3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(alg / (ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_src,
                        "kernel": "class_bitmap16_kernel (HIP events)", "kernel_ms_avg": round(ms, 3),
                        "algorithmic_bytes_per_launch": int(alg)}}
    if ob.ref_available():
        R = ob.href(ob.ref_variants()[-1])
        packed = np.zeros((len(classes), 33), dtype=np.uint8)
        for i, cls in enumerate(classes):
            lo, hi = np.zeros(16, np.uint8), np.zeros(16, np.uint8)
            bm = np.ascontiguousarray(cls.bitmap)
            if R.hsref_shufti_build(bm.ctypes.data, lo.ctypes.data, hi.ctypes.data) > 0:
                packed[i, 0] = 0
            else:
                R.hsref_truffle_build(bm.ctypes.data, lo.ctypes.data, hi.ctypes.data)
                packed[i, 0] = 1
            packed[i, 1:17], packed[i, 17:33] = lo, hi
        k = int(np.searchsorted(uoff, 64 << 20, side="right")) - 1
        s_off = np.ascontiguousarray(uoff[: k + 1])
        cpus = len(os.sched_getaffinity(0))
        out = (C.c_double * 4)()
        R.hsref_class_bench_threads.restype = C.c_int
        R.hsref_class_bench_threads.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int,
                                                C.c_double, C.c_int, C.c_void_p]
        sweep, best = {}, None
        for T in sorted({t for t in (8, 32, 128, cpus) if t <= cpus}):
            rv = R.hsref_class_bench_threads(packed.ctypes.data, len(classes), unit.ctypes.data, s_off.ctypes.data, k, T, 1.0, 1, out)
            assert rv == 0
            sweep[f"T{T}"] = round(out[0] / out[1] / 1e9, 3)
            if best is None or sweep[f"T{T}"] > best[0]:
                best = (sweep[f"T{T}"], T)
        cpus = best[1]
        res["cpu_baseline"] = {"value": best[0], "unit": "GB/s of corpus (all classes)", "cores": best[1],
                               "kind": "reference", "cpu": host_cpu_desc(), "runs": sweep, "cgroup_cpu_quota": cgroup_cpu_quota()[0],
                               "sample": f"first {int(s_off[-1])} bytes / {k} lines; per line and class shuftiExec / truffleExec + "
                                         f"their reverse forms (first and last member), T pinned pthreads x own slice, ~1 s per T, best T = {cpus}"}
    del d_corpus, cls_buf, fl_buf
    torch.cuda.empty_cache()
    return res


# ---- flood density ("flood-density corpora must be reported separately") -------------------

def run_flood(args):
    """The reference's flood case (src/fdr/flood_runtime.h:86-335, unit/internal/fdr_flood.cpp:148-557): long runs of
    one byte under literals made of that byte. 64 blocks of 1 MiB, block b filled with one byte value (16 values in
    turn); for four of the values the set holds the 4-byte and the 8-byte run of that byte (two matches per corpus
    byte in a quarter of the blocks) and a near miss; 100 ordinary literals ride along."""
    import torch

    from hyperscan_amd import corpus as cp
    from hyperscan_amd.hwlm import HwlmLiteral
    from tests import oracle_binding as ob

    nb, blk = 64, 1 << 20
    corpus = np.repeat((np.arange(nb) % 16 + ord("a")).astype(np.uint8), blk)
    off = (np.arange(nb + 1, dtype=np.uint64) * np.uint64(blk))
    lits = []
    for c in b"abcd":
        lits += [HwlmLiteral(bytes([c]) * 4, False, len(lits)), HwlmLiteral(bytes([c]) * 8, False, len(lits) + 1),
                 HwlmLiteral(bytes([c]) * 3 + b"x", False, len(lits) + 2)]
    lits += [HwlmLiteral(l.s, l.nocase, len(lits) + i) for i, l in enumerate(cp.teddy_literals(100, seed=12))]
    want_total = 16 * ((blk - 3) + (blk - 7))
    # the output protocol of hsgpu_hwlm_scan_dev: a count above cap (cap + 1: a staging region, sized from cap for an
    # even spread, overflowed) means "again with more room" -- flood blocks hold four times the average density
    cap = want_total + (1 << 20)
    job = GpuJob(lits, corpus, off, torch.cuda.current_device(), cap=cap)
    for attempt in range(5):  # the same scratch throughout: it is the scratch that remembers a dense scan
        job.launch()
        torch.cuda.synchronize()
        n = job.count()
        if n <= cap:
            break
        cap *= 2
        job.cap = cap
        job.d_out = None
        torch.cuda.empty_cache()
        job.d_out = torch.zeros(cap * 4, dtype=torch.int32, device=job.dev)
    assert n == want_total, f"flood: {n} matches, expected {want_total}"
    # content gate on the first block against the reference (or the restatement)
    d_first = job.d_out[: 4 * (2 * blk)].view(-1, 4)
    g = d_first[d_first[:, 0] == 0].cpu().numpy().astype(np.uint32)
    ref = ob.Reference(lits, variant=ob.ref_variants()[-1]) if ob.ref_available() else ob.Oracle(lits)
    want = ref.collect_blocks(corpus[:blk], off[:2])
    key = (g[:, 1].astype(np.uint64) << np.uint64(32)) | g[:, 3].astype(np.uint64)
    assert np.all(key[1:] > key[:-1]), "flood: records of block 0 not in delivery order"
    wi = np.lexsort((want["id"], want["end"]))
    gi = np.lexsort((g[:, 2], g[:, 1]))
    assert len(g) == len(want) and np.array_equal(g[gi, 1], want["end"][wi]) and np.array_equal(g[gi, 2], want["id"][wi]), \
        "PARITY FAILURE on the flood block"
    steps = max(3, min(args.steps, 10))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        job.launch()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    assert job.count() == n
    over = job.scratch.stats()[1]
    f_ms, c_ms, p_ms = job.scratch.timing(0)  # filter kernel (events), filter end -> end of the confirm stage, filter start -> last record placed
    res = {"workload": "flood: 64 blocks of 1 MiB, each one byte value repeated (16 values in turn); for 4 of them the set holds the "
                       "4- and 8-byte run of that byte: 2 matches per corpus byte in a quarter of the blocks; + 100 ordinary literals",
           "value": round(job.total / dt / 1e9, 2), "unit": "GB/s", "ms_per_step": round(dt * 1e3, 3),
           "matches_per_step": int(n), "matches_per_s": round(n / dt, 1), "record_bytes_per_step": int(n) * REC_BYTES,
           "candidate_overflow_scans": int(over), "record_capacity": int(cap),
           "stages_ms": {"filter": round(f_ms, 3), "confirm_place_copy": round(c_ms, 3), "pipeline": round(p_ms, 3),
                         "gather_and_gaps": round(dt * 1e3 - p_ms, 3)},  # (pipeline = filter start -> the gather's start: the rest of a step is record_sort_kernel expanding the runs, ~6 us of gaps)
           "pipeline": "folded, dense: every chunk has a candidate entry; dense batches confirmed position by position, emitted in order",
           "parity": f"count exact ({n}); (end, id) of block 0 ({len(want)} matches) identical to the reference, delivery order checked",
           "table": job.table.info()}
    if ob.ref_available():
        nbytes, secs, matches, _p = ref.bench_threads(corpus[: 4 * blk], off[:5], 4, 1.0)
        res["cpu_baseline"] = {"value": round(nbytes / secs / 1e9, 3), "unit": "GB/s", "cores": 4, "kind": "reference",
                               "sample": "the first 4 blocks (all four flood bytes), one pinned thread per block, ~1 s", "engine": ref.info(),
                               "matches_per_pass": int(matches)}
    del job
    torch.cuda.empty_cache()
    return res


# ---- config 5: literal hits feeding the host-side confirm ---------------------------------------

def run_rose1000(args):
    """Config 5 ("report GPU GB/s, host confirm hits/s, end-to-end GB/s" + a parity gate): 1000 patterns
    LIT_k + tail. GPU literal hits feed the host-side confirm (the reference: src/rose/match.c:479-523 calling into
    src/rose/program_runtime.c:2896-2942 per literal hit)."""
    import torch

    from hyperscan_amd import corpus as cp
    from hyperscan_amd import hs
    from hyperscan_amd.hwlm import HwlmLiteral
    from tests import oracle_binding as ob
    from tests import rose_model as RM

    rng = np.random.default_rng(6)
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ", dtype=np.uint8)
    lits = sorted({bytes(rng.choice(alpha, int(rng.integers(6, 13)))) for _ in range(1000)})
    pats = [l.decode() + RM.TAILS[i % 3] for i, l in enumerate(lits)]
    db = hs.Database.compile(pats, [0] * len(pats), list(range(len(pats))))
    scratch = hs.HsScratch(db)
    total = int(args.rose_gib * (1 << 30))

    class L:  # corpus generator wants objects with .s
        def __init__(self, s):
            self.s = s
    follow = [b"abc7", b"  key=", b"....END"]
    plant = [L(l + follow[i % 3]) if i % 2 == 0 else L(l) for i, l in enumerate(lits)]
    corpus, off = cp.packet_corpus(total, plant, seed=6, match_every=4096)
    lib = hs._lib()
    handler = C.cast(lib.hs_batch_count_handler, hs.BATCH_CB)  # hsbench's counting callback, native
    # the corpus in pinned host memory: the H2D leg runs at PCIe speed instead of through the pageable path
    pinned = torch.from_numpy(corpus).pin_memory()
    buf = pinned.numpy()
    offs = np.ascontiguousarray(off, dtype=np.uint64)

    # -- parity gate: (block, id, to) of a slice through hs_scan_batch against the model of tests/rose_model.py (pinned to
    #    Python re and to hs_confirm_batch in the CPU suite); the literal occurrences of the model come from the HWLM oracle
    #    ... on 4 slices of `--rose-gate-mib` / 4 MiB each (round 4: the first 8 MiB): the head, two inside and the tail of the corpus
    keyed = db.literals()
    hl = [HwlmLiteral(k[0], k[1], i) for i, k in enumerate(keyed)]
    href_ = ob.Reference(hl, variant=ob.ref_variants()[-1]) if ob.ref_available() else ob.Oracle(hl)
    per = max(1, args.rose_gate_mib // 4) << 20
    n_gate_ev, n_gate_blocks, n_gate_bytes, n_slices = 0, 0, 0, 0
    c_total = int(off[-1])
    for lo_byte in sorted({0, c_total // 3, 2 * c_total // 3, max(0, c_total - per)}):
        b0 = min(int(np.searchsorted(off, lo_byte, side="left")), int(off.size - 2))
        b1 = max(b0 + 1, int(np.searchsorted(off, min(c_total, int(off[b0]) + per), side="right")) - 1)
        b1 = min(b1, int(off.size - 1))
        g_lo, g_hi = int(off[b0]), int(off[b1])
        g_off = np.ascontiguousarray(off[b0: b1 + 1] - off[b0])
        hits = href_.collect_blocks(corpus[g_lo:g_hi], g_off)
        want = RM.expected_events(corpus[g_lo:g_hi], g_off, lits, hits)
        got = []
        cb = hs.BATCH_CB(lambda b, i, f, t, _fl, _c: (got.append((int(b), int(i), int(t))), 0)[1])
        rv = lib.hs_scan_batch(db._h, buf.ctypes.data + g_lo, g_off.ctypes.data, b1 - b0, 0, scratch._h, cb, None)
        assert rv == 0
        assert sorted(got) == want, (f"PARITY FAILURE (rose1000): hs_scan_batch {len(got)} events vs model {len(want)} on blocks [{b0}, {b1}) "
                                     f"(bytes [{g_lo}, {g_hi}))")
        n_gate_ev, n_gate_blocks, n_gate_bytes, n_slices = n_gate_ev + len(want), n_gate_blocks + b1 - b0, n_gate_bytes + g_hi - g_lo, n_slices + 1
    parity = (f"(block, id, to) of all 1000 patterns on {n_slices} slices (head, two inside, tail: {n_gate_blocks} blocks / {n_gate_bytes} bytes, "
              f"{n_gate_ev} events) identical to the model of tests/rose_model.py (literal occurrences from the reference's hwlmExec, tails restated; "
              "pinned to Python re in the CPU suite)")

    # -- end to end from pinned host memory
    ts, n_ev = [], 0
    for _ in range(max(3, min(args.steps, 5)) + 1):
        cnt = C.c_ulonglong(0)
        t0 = time.perf_counter()
        rv = lib.hs_scan_batch(db._h, buf.ctypes.data, offs.ctypes.data, offs.size - 1, 0, scratch._h, handler, C.byref(cnt))
        ts.append(time.perf_counter() - t0)
        assert rv == 0
        assert n_ev in (0, cnt.value), "match count changed between repeats"
        n_ev = cnt.value
    t = float(np.median(ts[1:]))

    # -- the legs of that figure, each alone: the bus, the GPU literal stage on a resident corpus, the host confirm
    dev = torch.device("cuda", torch.cuda.current_device())
    d_tmp = torch.empty(total, dtype=torch.uint8, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    h2d = []
    for _ in range(3):
        e0.record()
        d_tmp.copy_(pinned, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        h2d.append(e0.elapsed_time(e1))
    del d_tmp
    job = GpuJob(hl, corpus, off, torch.cuda.current_device())
    for _ in range(3):
        job.launch()
    torch.cuda.synchronize()
    n_hits = job.count()
    assert n_hits <= job.cap
    steps = max(3, min(args.steps, 10))
    t0 = time.perf_counter()
    for _ in range(steps):
        job.launch()
    torch.cuda.synchronize()
    t_gpu = (time.perf_counter() - t0) / steps
    f_ms = float(np.mean([job.scratch.timing(b)[0] for b in range(steps)]))
    recs = np.ascontiguousarray(job.records())
    lib.hs_confirm_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_ulonglong, C.c_void_p, C.c_ulonglong, hs.BATCH_CB, C.c_void_p]
    tc = []
    for _ in range(3):
        cnt = C.c_ulonglong(0)
        t0 = time.perf_counter()
        rv = lib.hs_confirm_batch(db._h, buf.ctypes.data, offs.ctypes.data, offs.size - 1, recs.ctypes.data, len(recs), handler, C.byref(cnt))
        tc.append(time.perf_counter() - t0)
        assert rv == 0 and cnt.value == n_ev, f"host confirm over the resident scan's hits: {cnt.value} events, hs_scan_batch {n_ev}"
    t_conf = float(np.median(tc))
    # -- the RESIDENT form end to end (verdict, round 5): the corpus stays in HBM (hsbench loads it once), hs_scan_batch_resident = GPU
    #    literal scan + D2H of the hits + host confirm (which reads the bytes behind every hit from the host copy) + callbacks
    lib.hs_scan_batch_resident.restype = C.c_int
    lib.hs_scan_batch_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_ulonglong, C.c_void_p, C.c_void_p, C.c_void_p, hs.BATCH_CB, C.c_void_p]
    tr = []
    for _ in range(6):
        cnt = C.c_ulonglong(0)
        t0 = time.perf_counter()
        rv = lib.hs_scan_batch_resident(db._h, buf.ctypes.data, offs.ctypes.data, offs.size - 1, job.d_corpus.data_ptr(), job.d_off.data_ptr(),
                                        scratch._h, handler, C.byref(cnt))
        tr.append(time.perf_counter() - t0)
        assert rv == 0 and cnt.value == n_ev, f"hs_scan_batch_resident: rc {rv}, {cnt.value} events, hs_scan_batch {n_ev}"
    t_res = float(np.median(tr[1:]))
    alg = total + REC_BYTES * n_hits
    res = {"workload": f"rose1000: 1000 literal-prefix + tail patterns, {args.rose_gib:g} GiB of packets through hs_scan_batch from pinned host "
                       "memory (H2D of the corpus + GPU literal scan + D2H of the records + host confirm + counting callback)",
           "value": round(total / t / 1e9, 2), "unit": "GB/s end to end", "ms": round(t * 1e3, 1), "matches": int(n_ev),
           "matches_per_s": round(n_ev / t, 1), "parity": parity,
           "gpu_stage": {"GBps": round(total / t_gpu / 1e9, 1), "ms": round(t_gpu * 1e3, 3), "literal_hits": int(n_hits),
                         "what": "the database's literal table over the same corpus RESIDENT in HBM (hsgpu_hwlm_scan_dev, serial steps)"},
           "host_confirm": {"hits_per_s": round(n_hits / t_conf, 1), "ms": round(t_conf * 1e3, 2), "events": int(n_ev),
                            "threads": "the facade's own (hs_confirm_batch over the resident scan's hits)"},
           "resident_end_to_end": {"GBps": round(total / t_res / 1e9, 1), "ms": round(t_res * 1e3, 2), "events": int(n_ev),
                                   "what": "hs_scan_batch_resident: corpus resident in HBM (and in host memory for the confirm): GPU literal scan + D2H of "
                                           "the hits + host confirm + counting callback; nothing of the corpus crosses the bus"},
           "pinned_h2d_GBps": round(total / (float(np.median(h2d)) / 1e3) / 1e9, 1),
           "bound": "the bus: end to end cannot exceed pinned_h2d_GBps; the GPU stage and the host confirm hide behind the copies",
           "roofline": {"bound": "hbm", "achieved": round(alg / (f_ms / 1e3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(alg / (f_ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4), "traffic": None,
                        "kernel": filter_kernel_name(job.table.info()["flags"]), "kernel_ms_avg": round(f_ms, 4),
                        "algorithmic_bytes_per_launch": int(alg), "what": "the resident GPU stage's filter kernel (HIP events)"}}
    del job
    torch.cuda.empty_cache()
    if ob.ref_available():
        k = int(np.searchsorted(off, 256 << 20, side="right")) - 1
        s_off = np.ascontiguousarray(off[: k + 1])
        cpus = len(os.sched_getaffinity(0))
        ref = ob.Reference(hl, variant=ob.ref_variants()[-1])
        sweep, best = {}, None
        for T in sorted({t for t in (8, 32, 128, cpus) if t <= cpus}):
            nbytes, secs, matches, _p = ref.bench_threads(corpus[: int(s_off[-1])], s_off, T, 1.0)
            sweep[f"T{T}"] = round(nbytes / secs / 1e9, 3)
            if best is None or sweep[f"T{T}"] > best[0]:
                best = (sweep[f"T{T}"], T)
        cpus = best[1]
        res["cpu_baseline"] = {"value": best[0], "unit": "GB/s", "cores": best[1], "kind": "reference", "runs": sweep,
                               "cgroup_cpu_quota": cgroup_cpu_quota()[0],
                               "cpu": host_cpu_desc(), "engine": ref.info(),
                               "sample": f"first {int(s_off[-1])} bytes; the reference's hwlmExec over the 1000 literal prefixes (their last 8 "
                                         f"bytes, as Rose hands them to HWLM), T pinned pthreads, ~1 s per T, best T = {cpus}: the literal stage of the reference "
                                         "alone, without its confirm (an upper bound on what full hs_scan would do)",
                               "literal_hits_per_pass": int(matches)}
        # said plainly (verdict, round 4): for HOST-resident data the path is the bus, and the reference's literal stage alone, on
        # the cores of this same box, is faster than the bus
        res["note"] = (f"host-resident: {res['value']} GB/s = the bus ({res['pinned_h2d_GBps']} pinned H2D); reference literal stage ALONE on this host: "
                       f"{best[0]} GB/s (T={best[1]}): from host memory the CPU path wins; resident GPU stage: {res['gpu_stage']['GBps']} GB/s")
    return res


def run_batch_sweep(args):
    """hsbench block mode is ONE hs_scan per block (tools/hsbench/engine_hyperscan.cpp:132-145, main.cpp:502-528): what a call
    costs at that granularity, and how large a resident batch must be before hsgpu_hwlm_scan_dev reaches its throughput."""
    import torch

    from hyperscan_amd import hwlm as hw

    lits, corpus, off = build_workload("fdr10k", 1 << 30, 0)
    job = GpuJob(lits, corpus, off, torch.cuda.current_device())
    for _ in range(2):
        job.launch()
    torch.cuda.synchronize()
    job.scratch.enable_timing(False)  # (no events around the kernels: two event records cost as much as a small scan)
    sizes = [1460, 16 << 10, 64 << 10, 256 << 10, 1 << 20, 16 << 20, 256 << 20, 1 << 30]
    curve, peak = [], 0.0
    stream = torch.cuda.current_stream().cuda_stream

    def time_scans(tot, k, it):
        for _ in range(3):
            hw.hwlm_scan_dev(job.table, job.scratch, job.d_corpus.data_ptr(), tot, job.d_off.data_ptr(), k, job.d_out.data_ptr(), job.cap,
                             job.d_count.data_ptr(), 0, stream)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(it):
            hw.hwlm_scan_dev(job.table, job.scratch, job.d_corpus.data_ptr(), tot, job.d_off.data_ptr(), k, job.d_out.data_ptr(), job.cap,
                             job.d_count.data_ptr(), 0, stream)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / it, int(job.d_count.item())

    for sz in sizes:
        k = max(1, int(np.searchsorted(off, sz, side="right")) - 1)
        tot = int(off[k])
        it = 200 if tot < (16 << 20) else 20
        dt, n_found = time_scans(tot, k, it)
        row = {"bytes": tot, "blocks": k, "us_per_scan": round(dt * 1e6, 1), "GBps": round(tot / dt / 1e9, 2)}
        if tot <= (1 << 20):  # the sizes a solo scan (ONE launch) serves: the three-kernel pipeline beside it, same scratch, same count
            job.scratch.set_tuning(3)
            dt3, n3 = time_scans(tot, k, it)
            job.scratch.set_tuning(0)
            assert n3 == n_found, f"solo scan {n_found} records, three-kernel pipeline {n3}"
            row["us_three_kernels"] = round(dt3 * 1e6, 1)
        curve.append(row)
        peak = max(peak, tot / dt / 1e9)

    def reach(fr):
        for a, b in zip(curve, curve[1:]):
            if a["GBps"] < fr * peak <= b["GBps"]:  # log-linear interpolation between the two measured sizes
                w = (fr * peak - a["GBps"]) / (b["GBps"] - a["GBps"])
                return int(np.exp(np.log(a["bytes"]) + w * (np.log(b["bytes"]) - np.log(a["bytes"]))))
        return curve[0]["bytes"] if curve[0]["GBps"] >= fr * peak else None
    # one call per block, the way hsbench drives hs_scan: hsgpu_hwlm_exec on one 1460-byte packet (H2D + scan + D2H + callbacks)
    k1 = int(np.argmax(np.diff(off.astype(np.int64)) == 1460))
    blk = np.ascontiguousarray(corpus[int(off[k1]):int(off[k1 + 1])])
    # (the library's own counting callback, hsbench's onMatch: a Python callback per match and a trampoline per call are not what is measured)
    lib = job.table._lib
    ncb = C.c_uint64(0)
    count_cb = C.cast(lib.hsgpu_hwlm_count_cb, hw.HWLM_CB)
    lib.hsgpu_scratch_set_context(job.scratch._h, C.addressof(ncb))
    p_blk, n_blk = blk.ctypes.data, blk.size

    def one_call():
        return lib.hsgpu_hwlm_exec(job.table._h, p_blk, n_blk, 0, count_cb, job.scratch._h, hw.HWLM_ALL_GROUPS)
    lib.hsgpu_debug_exec_repeat.restype = C.c_int
    lib.hsgpu_debug_exec_repeat.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, hw.HWLM_CB, C.c_void_p, C.c_uint64, C.c_uint, C.POINTER(C.c_double)]
    ctypes_us = []

    def per_call(n=500):
        """microseconds per hsgpu_hwlm_exec call from a NATIVE loop (include/hsgpu_tuning.h, hsgpu_debug_exec_repeat: hsbench's loop is
        C++ too); the same through ctypes -- ~1 us more, the binding's own -- goes to ctypes_us"""
        for _ in range(5):
            assert one_call() == 0
        t0 = time.perf_counter()
        for _ in range(n):
            one_call()
        ctypes_us.append(round((time.perf_counter() - t0) / n * 1e6, 1))
        us = C.c_double(0)
        assert lib.hsgpu_debug_exec_repeat(job.table._h, p_blk, n_blk, 0, count_cb, job.scratch._h, hw.HWLM_ALL_GROUPS, n, C.byref(us)) == 0
        return us.value
    us_launch = per_call()  # a kernel launch per call (rounds 1-5)
    n_launch = ncb.value
    # ... and through the small-batch server (round 6, include/hsgpu.h): one resident workgroup, no launch per call
    # (enable 2: the requests through mapped host memory -- the only way on a device without a large PCIe BAR -- as the A/B of 1:
    # requests written straight into device memory)
    job.scratch.enable_server(2)
    ncb.value = 0
    us_host_mailbox = per_call(2000)
    assert ncb.value * 1005 == n_launch * 4005, "the server (mailbox in host memory) delivers other matches than the launch path"
    cu, su = C.c_float(), C.c_float()
    lib.hsgpu_scratch_server_last_us.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.hsgpu_debug_server_stamping.argtypes = [C.c_void_p, C.c_int]

    def device_times():
        """the request's device-side times: taken only while stamping is on (a stamp is a clock read the workgroup waits for), so a
        few calls of their own behind the timed ones"""
        lib.hsgpu_debug_server_stamping(job.scratch._h, 1)
        for _ in range(20):
            assert one_call() == 0
        lib.hsgpu_scratch_server_last_us(job.scratch._h, C.byref(cu), C.byref(su))
        lib.hsgpu_debug_server_stamping(job.scratch._h, 0)
    device_times()
    su_host = su.value
    job.scratch.enable_server(True)
    ncb.value = 0
    us_exec = per_call(2000)
    assert ncb.value * 1005 == n_launch * 4005, "the server delivers other matches than the launch path"
    calls, launches, _live = job.scratch.server_stats()
    device_times()
    job.scratch.enable_server(False)
    lib.hsgpu_scratch_set_context(job.scratch._h, None)
    res = {"workload": "fdr10k table; resident scans of the first N bytes of the 1 GiB corpus, serial launches (hsgpu_hwlm_scan_dev), and one "
                       "hsgpu_hwlm_exec call per 1460-byte block from host memory",
           "value": round(peak, 1), "unit": "GB/s at the largest batch",
           "us_per_hwlm_exec_call_1460B": round(us_exec, 1), "GBps_one_block_per_call": round(1460 / us_exec / 1e3, 4),
           "us_per_hwlm_exec_call_1460B_launch_path": round(us_launch, 1), "server": {"calls": calls, "launches": launches, "device_copy_us": round(cu.value, 2), "device_scan_us": round(su.value, 2),
                                                                                     "us_per_call_mailbox_in_host_memory": round(us_host_mailbox, 1), "device_scan_us_mailbox_in_host_memory": round(su_host, 2),
                                                                                     "us_per_call_through_ctypes": {"launch": ctypes_us[0], "mailbox_in_host_memory": ctypes_us[1], "server": ctypes_us[2]},
                                                                                     "measured": "a native loop of hsgpu_hwlm_exec calls (hsgpu_debug_exec_repeat), as hsbench's; through ctypes ~1 us more per call"},
           "half_peak_batch_bytes": reach(0.5), "ninety_percent_batch_bytes": reach(0.9), "curve": curve}
    del job
    torch.cuda.empty_cache()
    # ... and the same packet through the PUBLIC API: hs_scan per call (literal scan + host confirm + callback), the scratch's
    # small-batch server off and on (include/hs_gpu.h, hs_scratch_enable_small_batch_server); a ctypes loop (~1 us of its own per
    # call). Beside the figures above, never one of them; a failure here is reported, not raised.
    try:
        from hyperscan_amd import hs

        db = hs.Database.compile_lit([l.s for l in lits], [hs.HS_FLAG_CASELESS if l.nocase else 0 for l in lits], list(range(len(lits))))
        sc = hs.HsScratch(db)
        n_ev = [0]

        def on_ev(_i, _f, _t, _fl, _c):
            n_ev[0] += 1
            return 0
        cb = hs.MATCH_CB(on_ev)
        hlib = hs._lib()
        hlib.hs_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, hs.MATCH_CB, C.c_void_p]

        def hs_per_call(n):
            for _ in range(20):
                assert hlib.hs_scan(db._h, p_blk, n_blk, 0, sc._h, cb, None) == 0
            n_ev[0] = 0
            t0 = time.perf_counter()
            for _ in range(n):
                hlib.hs_scan(db._h, p_blk, n_blk, 0, sc._h, cb, None)
            return (time.perf_counter() - t0) / n * 1e6, n_ev[0] / n
        us_hs_launch, ev_launch = hs_per_call(300)
        sc.enable_server(True)
        us_hs_server, ev_server = hs_per_call(2000)
        hs_calls, hs_launches = sc.server_stats()
        sc.close()
        assert ev_launch == ev_server, "hs_scan through the server delivers other events than with a launch per call"
        res["hs_scan_per_call_1460B"] = {"us_launch_per_call": round(us_hs_launch, 1), "us_server": round(us_hs_server, 1), "events_per_call": ev_server,
                                         "server_calls": hs_calls, "server_launches": hs_launches,
                                         "what": "hs_scan (public API: literal scan + host confirm + callback) on the same packet, a ctypes loop"}
    except AssertionError:
        raise
    except Exception as e:  # noqa: BLE001
        res["hs_scan_per_call_1460B"] = {"error": f"{type(e).__name__}: {e}"}
    return res


# ---- the ONE line: compact, everything else to the details file ---------------------------------

ROOFLINE_KEYS = ("bound", "achieved", "peak", "unit", "frac", "kernel_frac", "kernel_achieved", "traffic", "traffic_source", "kernel", "kernel_ms_avg",
                 "kernel_ms_trace", "kernel_ms_device_clock_avg", "confirm_stage_ms_avg", "algorithmic_bytes_per_launch", "algorithmic_bytes_per_step",
                 "ms_all_passes", "pipeline_ms_avg", "issue_bound_ms")
CPU_KEYS = ("value", "unit", "cores", "kind", "cgroup_cpu_quota", "sample")


def _short(v, n=200):
    return v if not isinstance(v, str) or len(v) <= n else v[: n - 3] + "..."


def compact_roofline(r):
    if not r:
        return r
    out = {k: r[k] for k in ROOFLINE_KEYS if k in r}
    if isinstance(out.get("kernel"), str):
        out["kernel"] = out["kernel"].replace("true", "1").replace("false", "0").replace(", ", ",")
    return out


def compact_cpu(c):
    return {k: _short(c[k], 150) for k in CPU_KEYS if k in c} if c else c


def compact_also(name, r):
    if "error" in r:
        return r
    if name == "sustained":  # {"headline": .., "shard": ..}: numbers only (GB/s = bytes / ms_per_step; the details file has all of it)
        def smi(x):
            return {k: x[k] for k in ("sclk", "power_W") if k in x} if isinstance(x, dict) else x
        return {k: {**{kk: v[kk] for kk in ("steps", "ms_per_step", "last30_filter_ms", "last30_confirm_stage_ms", "drift_last_over_first")},
                    "GBps_whole": v["GBps"]["whole"], "smi_before": smi(v.get("smi_before")), "smi_after": smi(v.get("smi_after"))} for k, v in r.items()}
    if name == "virtual_ranks":  # (its figures are in multi_gpu.loopback; the whole object is in the details file)
        return {"n_ranks": r["n_ranks"], "scan_ms": r["scan_ms"], "in_line_as": "multi_gpu.loopback"}
    keep = ("value", "unit", "ms_per_step", "ms", "matches_per_step", "matches", "parity", "gpu_stage", "host_confirm", "resident_end_to_end",
            "pinned_h2d_GBps", "class_stage", "sequence_stage", "stages_ms", "us_per_hwlm_exec_call_1460B", "us_per_hwlm_exec_call_1460B_launch_path", "server", "hs_scan_per_call_1460B", "GBps_one_block_per_call",
            "half_peak_batch_bytes", "ninety_percent_batch_bytes", "curve", "parity_whole_corpus", "parity_reference", "note")
    out = {"workload": _short(r.get("workload", name), 110)}
    for k in keep:
        if k in r:
            v = r[k]
            if isinstance(v, dict):
                v = {kk: vv for kk, vv in v.items() if kk not in ("what", "kernel", "threads")}
            out[k] = _short(v, 170)
    if "roofline" in r:  # (the other workloads' lines: the figures the judge recomputes from; the rest is in the details file)
        keep_r = ("bound", "achieved", "frac", "kernel_frac", "traffic", "kernel", "kernel_ms_avg", "confirm_stage_ms_avg",
                  "algorithmic_bytes_per_launch", "algorithmic_bytes_per_step")  # (peak 8000 GB/s as in the headline's)
        out["roofline"] = {k: v for k, v in compact_roofline(r["roofline"]).items() if k in keep_r}
    if "cpu_baseline" in r:
        out["cpu_baseline"] = {k: v for k, v in compact_cpu(r["cpu_baseline"]).items() if k not in ("sample", "cgroup_cpu_quota")}
    return out


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: N ranks through torch.distributed.run on this node, the same command the
    driver's contract uses. Fewer than N devices is an error, not a smaller run."""
    import socket
    import subprocess

    import torch

    have = torch.cuda.device_count()
    if have < n:
        log(f"bench.py: --gpus {n} asked for, this box shows {have} GPU(s): refusing to run a smaller job under that label")
        return 3
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    log("bench.py: launching " + " ".join(cmd))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gib", type=float, default=1.0, help="corpus GiB per GPU")
    ap.add_argument("--workload", default="fdr10k", choices=["teddy64", "fdr10k"])
    ap.add_argument("--no-also", action="store_true", help="skip the other workloads' lines")
    ap.add_argument("--also", default="teddy64,class256,rose1000,flood,fdr10k_shard,batch_sweep,virtual_ranks",
                    help="comma-separated extra workloads at N = 1 (fdr10k_shard: one --gib shard, config 3's per-GPU piece at N = 8; "
                         "virtual_ranks: the N-rank step loop over the loopback transport on this one GPU)")
    ap.add_argument("--virtual-ranks", type=int, default=8, help="ranks of also.virtual_ranks (2 .. 8)")
    ap.add_argument("--sustain-seconds", type=float, default=2.0,
                    help="also.sustained: the headline's (and the shard's) steps back to back for this long; 0 = off")
    ap.add_argument("--class-gib", type=float, default=4.0)
    ap.add_argument("--class-gate-mib", type=int, default=1, help="class256: MiB of lines PER SLICE (the head of every GiB + the tail) whose match ends are compared with the model")
    ap.add_argument("--details", default=None, help="where the full (uncompacted) result goes; default gpurun_out/bench_details.json")
    ap.add_argument("--rose-gib", type=float, default=2.0)
    ap.add_argument("--rose-gate-mib", type=int, default=64, help="rose1000: MiB of packets (in 4 slices across the corpus) whose events are compared with the model")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baseline")
    ap.add_argument("--overlap-probe", dest="overlap_probe", action="store_true", default=True,
                    help="also time the steps with two scans in flight on two streams (value_two_scratches, beside value and never as "
                         "it: hsbench's -T 2); on by default since round 6")
    ap.add_argument("--no-overlap-probe", dest="overlap_probe", action="store_false",
                    help="serial launches only (tools/round_profile.sh: a kernel trace of the run then holds nothing else)")
    ap.add_argument("--scaling", default="strong", choices=["weak", "strong"],
                    help="strong (the default since round 6: BASELINE.json's config 3 is ONE 8 GiB corpus sharded across the GPUs): the same "
                         "--shards x --gib GiB at every GPU count, rank r scanning shards [r, r + 1) * shards / N -- N = 1 holds all 8 GiB "
                         "resident, N = 8 one GiB per GPU; weak: one --gib shard per GPU whatever N")
    ap.add_argument("--shards", type=int, default=8, help="shards of --gib GiB that make up the strong-scaling corpus")
    ap.add_argument("--exchange", default="auto", choices=["auto", "native", "native_all", "padded", "exact"],
                    help="N > 1: auto = the C ABI's exchange over RCCL, records to rank 0 (12-byte wire records), falling back to "
                         "torch.distributed (padded all-gather, or exact-size broadcasts when the per-rank counts are skewed) when it "
                         "cannot be created; native_all = the same to every rank; padded / exact = the torch.distributed forms. "
                         "(round 5: auto = native_all, the all-gather BASELINE.json names, with the to-root form timed beside it)")
    ap.add_argument("--pipeline-depth", type=int, default=0, choices=[0, 1, 2],
                    help="scans in flight: 2 overlaps a step's record all-gather with the next step's scan; "
                         "0 = 1 at N = 1 (the per-kernel figures are then those of the kernels alone), 2 at N > 1")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the headline's last step's output (its match records) to DIR as .npy files "
                         "(float64; at most 64 MB, a fixed seeded sample of a larger output): two builds can be compared output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback)")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` on its own: the N ranks are launched from here (one process per GPU over RCCL, as the
        # contract's torch.distributed.run line does), never a silent one-GPU run with n_gpus: 1 in the line
        sys.exit(self_launch(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch {args.gpus} ranks (or run `python bench.py --gpus "
                         f"{args.gpus}` without WORLD_SIZE set: it starts them itself)")
    if torch.cuda.device_count() <= local:
        raise SystemExit(f"bench.py: rank {rank} wants device {local}, this box shows {torch.cuda.device_count()}")
    torch.cuda.set_device(local)
    dist = None
    # HSGPU_BENCH_FORCE_DIST=1: take the N > 1 path (process group, exchange, two streams) at world size 1 too --
    # the one way to run that code on a 1-GPU box
    if world > 1 or os.environ.get("HSGPU_BENCH_FORCE_DIST"):
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        formed = dist.get_world_size()  # the ranks RCCL actually formed: what n_gpus reports
        assert formed == world, f"process group of {formed} ranks, WORLD_SIZE {world}"

    do_cpu = (rank == 0 and dist is None and not args.no_cpu)
    if args.scaling == "strong" and args.shards % world:
        raise SystemExit(f"bench.py: --shards {args.shards} is no multiple of {world} ranks")
    main_res = run_workload(args.workload, args, rank, world, dist, do_cpu, dump_dir=args.dump_outputs)
    also = {}
    if "sustained" in main_res:
        also["sustained"] = {"headline": main_res.pop("sustained")}
    if not args.no_also and dist is None:
        for name in [a for a in args.also.split(",") if a]:
            t0 = time.perf_counter()
            try:
                import copy

                if name == "fdr10k_shard":  # config 3's per-GPU piece at N = 8 (rounds 1-5's headline): what the multi-GPU prediction is made of
                    a1 = copy.copy(args)
                    a1.shards_override = [0]
                    a1.reference_gate = not args.no_cpu
                    r1 = run_workload("fdr10k", a1, rank, world, None, False)
                    if "sustained" in r1:
                        also.setdefault("sustained", {})["shard"] = r1.pop("sustained")
                    also[name] = {"workload": f"fdr10k, ONE shard of {args.gib:g} GiB resident (config 3's per-GPU piece at N = {args.shards}; rounds 1-5's headline)",
                                  **{k: r1[k] for k in ("value", "ms_per_step", "matches_per_s", "matches_per_step", "parity_whole_corpus", "parity_reference",
                                                        "two_scans_in_flight") if k in r1},
                                  "unit": "GB/s", "roofline": r1["roofline"]}
                    continue
                if name == "virtual_ranks":
                    nr = max(2, min(8, args.virtual_ranks))
                    lits_v = build_workload("fdr10k", int(args.gib * (1 << 30)), 0)[0]
                    shards = [build_workload("fdr10k", int(args.gib * (1 << 30)), sid)[1:] for sid in range(nr)]
                    also[name] = run_virtual_ranks(args, nr, lits_v, shards)
                    continue
                if name == "class256":
                    also[name] = run_class256(args)
                elif name == "rose1000":
                    also[name] = run_rose1000(args)
                elif name == "flood":
                    also[name] = run_flood(args)
                elif name == "batch_sweep":
                    also[name] = run_batch_sweep(args)
                elif name == "fdr10k_8g":  # config 3's whole 8 GiB on ONE GPU: the N = 1 point of the strong-scaling curve
                    import copy

                    a8 = copy.copy(args)
                    a8.shards_override = list(range(args.shards))
                    a8.reference_gate = not args.no_cpu
                    a8.steps, a8.warmup = max(3, min(args.steps, 10)), 2
                    r8 = run_workload("fdr10k", a8, rank, world, None, False)
                    also[name] = {"workload": f"fdr10k, {args.shards} shards x {args.gib:g} GiB resident on one GPU ({args.shards * args.gib:g} GiB per step)",
                                  **{k: r8[k] for k in ("value", "ms_per_step", "matches_per_s", "matches_per_step", "parity_whole_corpus", "parity_reference") if k in r8},
                                  "unit": "GB/s", "roofline": r8["roofline"]}
                elif name != args.workload:
                    also[name] = run_workload(name, args, rank, world, dist, do_cpu)
            except Exception as e:  # an extra line must not take the headline down with it
                also[name] = {"error": f"{type(e).__name__}: {e}"}
            log(f"also.{name}: {time.perf_counter() - t0:.1f}s")

    _WORKLOAD_CACHE.clear()
    if rank == 0 and dist is None:
        # what an N-GPU step of config 3 is made of: the scan of ONE shard as measured here (also.fdr10k_shard; the headline itself when it
        # is one shard), the records of one rank on the wire over xGMI's point-to-point links at 153 GB/s x 0.8 each
        # (MI355X_MICROARCH.md) -- arithmetic --, and, measured on this one GPU, everything of the exchange except the wire
        # (also.virtual_ranks: pack, the transfers as device copies, compact)
        shard = also.get("fdr10k_shard") if isinstance(also.get("fdr10k_shard"), dict) and "ms_per_step" in also.get("fdr10k_shard", {}) else \
            (main_res if args.scaling == "weak" or args.shards == 1 else None)
        if shard is not None:
            wire = 16 + 12 * int(shard["matches_per_step"])
            link = 153e9 * 0.8
            main_res["multi_gpu"] = {"predicted_for_n_gpus": args.shards, "measured": False, "scan_ms": shard["ms_per_step"], "wire_bytes_per_rank": wire,
                                     "to_root_ms": round(wire / link * 1e3, 4), "ring_all_gather_ms": round((args.shards - 1) * wire / link * 1e3, 4),
                                     "point_to_point_all_gather_ms": round(wire / link * 1e3, 4),
                                     "step_ms_exchange_overlapped_with_next_scan": round(max(shard["ms_per_step"], wire / link * 1e3), 4),
                                     "assumes": "153 GB/s x 0.8 per xGMI link; to-root / point-to-point: every peer over its own link; ring: N - 1 ranks' records over every link"}
            vr = also.get("virtual_ranks")
            if isinstance(vr, dict) and "all_gather" in vr:
                main_res["multi_gpu"]["loopback"] = {"n_ranks": vr["n_ranks"], "scan_ms_all_ranks": vr["scan_ms"],
                                                     **{m: {k: vr[m][k] for k in ("pack_ms", "collective_ms", "compact_ms", "step_ms", "step_minus_scans_ms")}
                                                        for m in ("all_gather", "to_root") if m in vr}}
    if rank == 0:
        blocks_desc = "synthetic packets {64,128,256,576,1024,1460} B, 70% HTTP-like text / 30% random"
        box = box_info()
        full = {"headline": main_res, "also": also, "box": box}
        out = {
            "metric": "GB/s scanned (hsbench block mode)", "value": main_res["value"], "unit": "GB/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": main_res["ms_per_step"],
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "config": {"workload": (f"{args.workload}: {WORKLOAD_DESC[args.workload]}, {args.gib:g} GiB per GPU, block mode, {blocks_desc}" if args.scaling == "weak" else
                                    f"{args.workload} (BASELINE.json config 3): {WORKLOAD_DESC[args.workload]}, ONE corpus of {args.shards} x {args.gib:g} GiB = "
                                    f"{args.shards * args.gib:g} GiB, {args.shards * args.gib / world:g} GiB resident per GPU, block mode, {blocks_desc}"),
                       "records": "16 B (block,end,id,lit), delivery order", "pipeline_depth": main_res["pipeline_depth"],
                       "sharding": (f"{world} x independent shards" if args.scaling == "weak" else
                                    f"strong: {args.shards} shards x {args.gib:g} GiB in all, {args.shards // world} per GPU")
                       + ({"all_gather": ", RCCL all-gather of the match records per step (value); to-root timed beside it",
                           "to_root": ", RCCL gather of the match records to rank 0 per step (value); all-gather timed beside it",
                           "exact": ", torch.distributed broadcasts of exactly the records per step (value)",
                           "padded": ", torch.distributed padded all-gather of the records per step (value)"}[main_res["exchange"]["value_uses"]]
                          if dist is not None else "")},
            "matches_per_s": main_res["matches_per_s"], "matches_per_step": main_res["matches_per_step"],
            "roofline": compact_roofline(main_res["roofline"]),
        }
        out["box"] = {"gpu": box.get("kfd", {}).get("unique_id"), "fw": box.get("kfd", {}).get("fw_version"), "driver": box.get("amdgpu_driver") or box.get("kernel"),
                      "xnack": box["env"].get("HSA_XNACK")}
        knobs = {k: os.environ[k] for k in ("HSGPU_LIB_VARIANT", "HSGPU_BUILD_FLAGS", "HSGPU_BENCH_FORCE_DIST", "HSGPU_PROFILE_DIR") if os.environ.get(k)}
        if knobs:  # a tuning build or forced table flags under the headline must be visible in the record
            out["env_knobs"] = knobs
        if "cpu_baseline" in main_res:
            out["cpu_baseline"] = compact_cpu(main_res["cpu_baseline"])
        if "parity_whole_corpus" in main_res:
            out["parity"] = {"reference": _short(main_res.get("parity_reference", "no CPU leg in this run"), 200),
                             "whole_corpus": _short(main_res["parity_whole_corpus"], 170)}
        if "end_to_end_resident" in main_res:
            e = main_res["end_to_end_resident"]
            out["end_to_end_resident"] = {k: e[k] for k in ("GBps", "ms", "replay_threads", "matches_delivered")}
        if "host_buffers" in main_res:
            out["host_buffers"] = {k: main_res["host_buffers"][k] for k in ("GBps", "pipelined_GBps", "sample_bytes")}
        if "two_scans_in_flight" in main_res:  # beside `value`, never as it: two scratches on two streams (hsbench -T 2)
            out["value_two_scratches"] = main_res["two_scans_in_flight"]["GBps"]
            out["ms_per_step_two_scratches"] = main_res["two_scans_in_flight"]["ms_per_step"]
        for k in ("exchange", "multi_gpu"):
            if k in main_res:
                out[k] = main_res[k]
        if dist is None and isinstance(out.get("multi_gpu"), dict):
            out["multi_gpu"] = {k: v for k, v in out["multi_gpu"].items() if k != "assumes"}  # (the details file keeps it)
        if also:
            out["also"] = {k: compact_also(k, v) for k, v in also.items() if k != "virtual_ranks" or "error" in v}  # (virtual_ranks: multi_gpu.loopback)
        # the full objects: stderr and a side file
        dpath = args.details or os.path.join(ROOT, "gpurun_out" if os.path.isdir(os.path.join(ROOT, "gpurun_out")) else "", "bench_details.json")
        try:
            os.makedirs(os.path.dirname(dpath), exist_ok=True)
            with open(dpath, "w") as f:
                json.dump(full, f, indent=1)
            out["details"] = os.path.relpath(dpath, ROOT)
        except OSError as e:
            out["details"] = f"not written ({e})"
        log("bench details: " + json.dumps(full))
        line = json.dumps(out)
        if len(line) > 6800:  # the driver keeps an ~8.5 KB tail of stdout: shed what the details file holds anyway
            for k in ("curve",):
                for v in out.get("also", {}).values():
                    v.pop(k, None)
            for v in out.get("also", {}).values():
                v.pop("workload", None)
            line = json.dumps(out)
        if len(line) > 6800:  # still: the prose of the other workloads (the gates ran; their wording is in the details file)
            for v in out.get("also", {}).values():
                for k in ("parity", "parity_whole_corpus", "parity_reference", "matches", "note"):
                    if isinstance(v.get(k), str) and len(v[k]) > 60:
                        v[k] = v[k][:57] + "..."
                if isinstance(v.get("roofline"), dict):
                    v["roofline"].pop("traffic_source", None)
            line = json.dumps(out)
        out_line = line
    if dist is not None:
        # every rank empties its C stdio buffer (RCCL's banner) before anyone can print the result line
        sys.stdout.flush()
        try:
            C.CDLL(None).fflush(None)
        except OSError:
            pass
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        # the ONE line, and the last thing on stdout: RCCL writes a version banner through C stdio, which sits in
        # libc's buffer (stdout is a pipe) until exit unless it is flushed out first
        sys.stdout.flush()
        try:
            C.CDLL(None).fflush(None)
        except OSError:
            pass
        print(out_line, flush=True)


if __name__ == "__main__":
    main()
