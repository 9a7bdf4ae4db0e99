#!/usr/bin/env python3
"""bench.py -- input GB/s of the LZS block-compression hot path on MI355X.

N = 1: a "step" is one pass of lzs_compress_batch_device over one batch of independent 64 KiB
blocks already resident in HBM (BASELINE.json configs[1]: 1 GiB = 16384 blocks of
enwik-style ASCII text).  A plain run sets up, warms up, times the steps and prints the line
(`value`, `ms_per_step`, and the roofline of the timed launches).  With --full, after the timed
region EVERY block is also compared with the reference C compressor on the host cores (which is
also the cpu_baseline), the other two classes are measured and checked the same way, and the
config-5 job below is run once more at world size 1 (`config5_world1`), so that the scaling
curve's first point has the same fields as the others.  --dump-outputs DIR writes what the last
timed step computed to DIR/*.npy (dump_outputs below), for comparing two builds output for output.

N > 1 (BASELINE.json configs[4]): 131072 blocks (8 GiB) per GPU --
64 GiB at 8 GPUs -- generated in HBM on the root GPU by lzs_gen_blocks_kernel; a "step" is the
whole job, pipelined over chunks of blocks (lzs_compression_amd/sharded_job.py): SCATTER (root ->
ranks, RCCL point-to-point over xGMI) || COMPRESS (every rank its shard; blocks are independent,
no collective) || GATHER (compaction + gather-v of the compressed streams and their lengths to the
root).  `value` is the end-to-end rate of the whole job; each phase is also timed alone, in one
un-overlapped pass after the timed region (`phases_ms`, `compute_only_GBps`, `scatter_GBps`,
`gather_GBps`).  Weak scaling: per-GPU work is fixed.

How it starts (the parent never touches the GPU):

    python bench.py                            # 1 GPU, in this process (the headline only)
    python bench.py --full                     # ... and every check and secondary figure
    python bench.py --gpus 8                   # no WORLD_SIZE in the environment: launches its own
                                               # 8 ranks (a child `python -m torch.distributed.run`)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
        --master-port 29500 bench.py --gpus 8  # the driver's way: every rank is a supervisor that
                                               # runs the job in a child process

If the RCCL job fails or hangs on any rank (first hardware run of the point-to-point legs), every
supervisor falls back to independent shards without any collective -- the compute-only
weak-scaling number, labelled as such (`fallback`) -- so an 8-GPU lease never ends with no number.

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BLOCK = 65536
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md, chip-level table)
METRIC = "input GB/s on 64KiB blocks, bit-exact vs C ref"
CLASS_NAMES = ("text", "lowent", "random")

np = torch = lzs = workload = None


def heavy_imports() -> None:
    """numpy / torch / the library: only in processes that do GPU work (never in a launcher or a
    supervisor, which must stay clean of the GPU so that they may start other programs)."""
    global np, torch, lzs, workload
    if lzs is None:
        import numpy as _np
        import torch as _torch
        import lzs_compression_amd as _lzs
        from lzs_compression_amd import workload as _workload
        np, torch, lzs, workload = _np, _torch, _lzs, _workload
        assert tuple(workload.CLASS_NAMES) == CLASS_NAMES


def usable_cores() -> int:
    """Host cores this process may really use: the smaller of the affinity mask and the
    cgroup CPU quota (the GPU box advertises 256 CPUs but grants a 16-CPU quota)."""
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            cores = min(cores, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return cores


def host_cpu() -> dict:
    """The host the cpu_baseline ran on ("state the count and CPU model"): the model name, the physical
    cores (distinct (package, core) pairs of /proc/cpuinfo), the logical CPUs of the affinity mask, and the cgroup's CPU
    quota in cores (None: unlimited) -- `cores` of the baseline is the smaller of the last two, what the threads can use."""
    model, pairs, phys, core = None, set(), None, None
    try:
        for ln in open("/proc/cpuinfo"):
            k, _, v = ln.partition(":")
            k, v = k.strip(), v.strip()
            if k == "model name" and model is None:
                model = v
            elif k == "physical id":
                phys = v
            elif k == "core id":
                core = v
            elif not k and phys is not None and core is not None:
                pairs.add((phys, core))
                phys = core = None
        if phys is not None and core is not None:
            pairs.add((phys, core))
    except OSError:
        pass
    quota = None
    try:
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            quota = int(q) / int(period)
    except (OSError, ValueError):
        pass
    return {"cpu_model": model, "physical_cores": len(pairs) or None,
            "logical_cpus": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count(), "quota_cores": quota}


def kernel_identity() -> str:
    """SHA-256 over the sources the measured kernel, lzs_compress_blocks_wg_kernel, is compiled from
    (kernels/common.inc, kernels/compress_wg.inc and kernels/compress_aux.inc: its code in every variant, its LDS
    layout, its launch geometry -- one workgroup of kWgThreads per block -- and the classifier that gives a block its
    variant; lzs_kernels.hip: what each variant's configuration is -- bucket counts, hops, sub-steps -- and the launcher):
    what a counter measurement belongs to.
    (The decoders' sources are not part of it: the traffic figure is the compress kernel's.)"""
    import hashlib
    csrc = os.path.join(ROOT, "lzs_compression_amd", "csrc")
    h = hashlib.sha256()
    for name in ("kernels/common.inc", "kernels/compress_wg.inc", "kernels/compress_aux.inc", "lzs_kernels.hip"):
        h.update(os.path.basename(name).encode() + b"\0" + open(os.path.join(csrc, name), "rb").read())
    return h.hexdigest()


def pmc_traffic(cls: str):
    """HBM bytes per launch from the committed rocprofv3 PMC passes (profiles/pmc_traffic.json,
    written by tools/gpu_traffic.sh), or (None, why).  The file carries the identity of the kernel
    sources it was measured on; with other sources in the tree the number is stale and not reported.
    FETCH_SIZE is doubled as MI355X_MICROARCH.md prescribes for gfx950 wide streaming reads."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        doc = json.load(open(path))
        rec = doc[cls]
    except (OSError, KeyError, ValueError):
        return None, "profiles/pmc_traffic.json has no entry for this class"
    if doc.get("kernel_source_sha256") != kernel_identity():
        return None, ("profiles/pmc_traffic.json was measured on other kernel sources (its kernel_source_sha256 differs "
                      "from this tree's): stale, not reported; regenerate with tools/gpu_traffic.sh")
    return {"hbm_bytes": rec["fetch_bytes_corrected"] + rec["write_bytes"], "kernel_source_sha256": doc["kernel_source_sha256"], **rec}, None


def host_codec():
    """(codec, kind): the reference C compressor (oracle/_ref, kind "reference") or, where it did not
    travel, our C restatement (kind "port")."""
    import oracle
    kind = "reference" if oracle.have_ref() else "port"
    return (oracle.ref() if kind == "reference" else oracle.oracle()), kind


def cpu_sample(blocks_host) -> tuple:
    """The host codec timed on a BOUNDED sample of the same blocks (about 15 core-seconds), one block per
    task on the usable host cores, and on one core.  Returns (the cpu_baseline object, the sample's
    streams, their lengths)."""
    import oracle
    cores = usable_cores()
    codec, kind = host_codec()
    nb = len(blocks_host)
    # size the timed sample for roughly 15 core-seconds of work: probe 64 blocks on one thread first
    _, _, probe = oracle.run_blocks(codec, blocks_host[:64], threads=1)
    per_block = max(probe / 64.0, 1e-6)
    nsample = int(min(nb, max(256, 15.0 / per_block)))
    out, out_len, secs = oracle.run_blocks(codec, blocks_host[:nsample], threads=cores)
    _, _, secs1 = oracle.run_blocks(codec, blocks_host[:max(64, nsample // cores)], threads=1)
    one_core = max(64, nsample // cores) * BLOCK / secs1 / 1e9
    return ({"value": nsample * BLOCK / secs / 1e9, "unit": "GB/s", "cores": cores, "kind": kind,
             **host_cpu(),
             "host": f"{os.cpu_count()} logical CPUs visible, {cores} usable (affinity/cgroup quota)",
             "one_core_GBps": one_core,
             "sample": f"first {nsample} of the same 64 KiB blocks ({nsample * BLOCK >> 20} MiB), "
                       f"one block per task, {cores} threads"}, out, out_len)


def check_every_block(blocks_host, gpu_len, gpu_slots, have=None) -> dict:
    """EVERY block of a launch compressed on the host and compared with the GPU's output, length and
    bytes (SURVEY.md 8d "every block compared"), in pieces of 2048 blocks (host memory stays small).
    `have` = (streams, lengths) of the first blocks if they were compressed already."""
    import hashlib
    import oracle
    cores = usable_cores()
    codec, kind = host_codec()
    nb = len(blocks_host)
    t_chk = time.perf_counter()
    exact, first_bad, compared = True, None, 0
    h_gpu, h_cpu = hashlib.sha256(), hashlib.sha256()
    for lo in range(0, nb, 2048):
        hi = min(nb, lo + 2048)
        if have is not None and hi <= len(have[1]):
            o, ol = have[0][lo:hi], have[1][lo:hi]
        else:
            o, ol, _ = oracle.run_blocks(codec, blocks_host[lo:hi], threads=cores)
        g = gpu_slots[lo:hi].cpu().numpy()
        gl = gpu_len[lo:hi]
        same_len = bool((ol == gl).all())
        for b in range(hi - lo):
            n = int(ol[b])
            gb, cb = g[b, :int(gl[b])], o[b, :n]
            h_gpu.update(gb.tobytes())
            h_cpu.update(cb.tobytes())
            if exact and (int(gl[b]) != n or not np.array_equal(gb, cb)):
                exact, first_bad = False, lo + b
        exact = exact and same_len
        compared += hi - lo
    exact = exact and h_gpu.digest() == h_cpu.digest()
    return {"bit_exact": exact, "blocks_compared": compared, "of": nb, "against": kind,
            "what": "length and every byte of every block against the host codec",
            "sha256_of_all_streams": h_gpu.hexdigest(), "first_differing_block": first_bad,
            "seconds": time.perf_counter() - t_chk}


def cpu_baseline(blocks_host, gpu_len, gpu_slots) -> dict:
    """The cpu_baseline object of the N = 1 line: the timed, bounded sample plus the unbounded check of
    every block of the launch against the same codec."""
    base, out, out_len = cpu_sample(blocks_host)
    chk = check_every_block(blocks_host, gpu_len, gpu_slots, have=(out, out_len))
    base["gpu_output_bit_exact_on_sample"] = chk["bit_exact"]
    base["check"] = chk
    return base


def pmc_limiter(cls: str):
    """What the committed counter passes say binds the kernel (profiles/pmc_limiter.json, written by
    tools/pmc_limiter.py from tools/gpu_pmc.sh's output), or (None, why): vector-issue and LDS busy
    fractions, bank-conflict share, vector instructions per input byte.  Guarded by the identity of the
    kernel sources like `traffic`."""
    path = os.path.join(ROOT, "profiles", "pmc_limiter.json")
    try:
        doc = json.load(open(path))
        rec = doc[cls]
    except (OSError, KeyError, ValueError):
        return None, "profiles/pmc_limiter.json has no entry for this class"
    if doc.get("kernel_source_sha256") != kernel_identity():
        return None, ("profiles/pmc_limiter.json was measured on other kernel sources: stale, not reported; "
                      "regenerate with tools/gpu_pmc.sh + tools/pmc_limiter.py")
    return dict(rec, kernel_source_sha256=doc["kernel_source_sha256"], how=doc.get("how")), None


DUMP_SAMPLE_BLOCKS = 128        # compressed blocks kept whole by --dump-outputs (128 x 73744 float32 = 38 MB)
DUMP_SAMPLE_SEED = 20240501


def dump_outputs(out_dir: str, slots, lens) -> dict:
    """--dump-outputs: what the caller of lzs_compress_batch_device received from the last timed step, as .npy files
    that two builds can be compared with, file for file:
      compressed_lengths.npy        float64 [nb]      every block's compressed length
      compressed_checksums.npy      float64 [nb]      every block's sum of byte[i] * (i + 1) over its compressed bytes
                                                      (exact: at most 255 * 73731 * 73732 / 2 < 2**53)
      compressed_sample_index.npy   float64 [S]       a fixed, seeded, sorted sample of S block indices
      compressed_sample.npy         float32 [S, stride] those blocks' slots, zero past each block's length
    Bytes past a block's length are not part of the output (the slots are not cleared), so they count nowhere."""
    os.makedirs(out_dir, exist_ok=True)
    nb, stride = slots.shape
    lens64 = lens.to(torch.int64)
    w = torch.arange(1, stride + 1, dtype=torch.int64, device=slots.device)
    sums = torch.empty(nb, dtype=torch.int64, device=slots.device)
    for lo in range(0, nb, 512):
        hi = min(nb, lo + 512)
        live = w[None, :] <= lens64[lo:hi, None]
        sums[lo:hi] = (slots[lo:hi].to(torch.int64) * w * live).sum(1)
    pick = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(nb, min(nb, DUMP_SAMPLE_BLOCKS), replace=False))
    idx = torch.from_numpy(pick).to(slots.device)
    sample = slots.index_select(0, idx)
    sample = sample * (torch.arange(stride, device=slots.device)[None, :] < lens64.index_select(0, idx)[:, None])
    arrays = {"compressed_lengths": lens64.cpu().numpy().astype(np.float64),
              "compressed_checksums": sums.cpu().numpy().astype(np.float64),
              "compressed_sample_index": pick.astype(np.float64),
              "compressed_sample": sample.cpu().numpy().astype(np.float32)}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {"dir": out_dir, "files": sorted(n + ".npy" for n in arrays), "bytes": int(sum(a.nbytes for a in arrays.values()))}


def emit(result: dict) -> None:
    """The ONE JSON line, last on stdout: RCCL writes a version banner through C stdio, which a pipe
    holds back until exit -- flush it out first."""
    import ctypes
    sys.stdout.flush()
    try:
        ctypes.CDLL(None).fflush(None)
    except OSError:
        pass
    print(json.dumps(result), flush=True)


# ============================================================================ launching (no GPU here)
def parse_args(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="text", choices=CLASS_NAMES)
    ap.add_argument("--blocks", type=int, default=None,
                    help="64 KiB blocks per GPU (default: 16384 = 1 GiB at N = 1, 131072 = 8 GiB at N > 1)")
    ap.add_argument("--chunk-blocks", type=int, default=8192,
                    help="N > 1: blocks per pipeline chunk of the scatter || compress || gather job (default 8192 = 512 MiB)")
    ap.add_argument("--no-overlap", action="store_true", help="N > 1: run the job un-overlapped (one chunk = the whole shard)")
    ap.add_argument("--check-every", type=int, default=16,
                    help="N > 1: the root compares the first 1/CHECK_EVERY and the last block of every chunk of every rank's "
                         "gathered streams with the CPU oracle (1 = every block)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-single-stream", action="store_true", help="skip the secondary single_stream line (profiling runs)")
    ap.add_argument("--no-other-classes", action="store_true",
                    help="N = 1: skip the other two 1 GiB classes (BASELINE.json configs[2], [3]) after the headline (profiling runs)")
    ap.add_argument("--no-config5", action="store_true", help="N = 1: skip the extra config5_world1 object (profiling runs)")
    ap.add_argument("--sharded-job", action="store_true",
                    help="run the N > 1 job (scatter / compress / gather over torch.distributed) even at N = 1: "
                         "exercises that code path with the nccl backend on a one-GPU box")
    ap.add_argument("--allow-shared-gpu", action="store_true",
                    help="ranks may share a GPU (LOCAL_RANK modulo the device count): for testing the launch and "
                         "fallback machinery on a one-GPU box; RCCL itself refuses two ranks on one device")
    ap.add_argument("--full", action="store_true",
                    help="N = 1: after the headline also measure and check everything else -- the device copy, the block "
                         "decoder, single_stream, the cpu_baseline with every block against the host codec, the other two "
                         "classes and config5_world1 (the --no-* switches above still drop single pieces).  Without it a "
                         "run sets up, warms up, times the steps and prints the line.  (N > 1 lines are the same either way.)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="N = 1: after the timed steps write what the last step computed to DIR/*.npy (e.g. bench_outputs/; float32 / float64, "
                         "under 64 MB): every block's compressed length and position-weighted byte sum, and the compressed "
                         "bytes of a fixed, seeded sample of blocks")
    return ap.parse_args(argv)


def free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def last_json_line(text: str):
    for ln in reversed(text.strip().splitlines()):
        ln = ln.strip()
        if ln.startswith("{") and ln.endswith("}"):
            try:
                doc = json.loads(ln)
            except ValueError:
                continue
            if "metric" in doc:
                return ln
    return None


def self_launch(args, argv) -> int:
    """`python bench.py --gpus N` with N > 1 and no WORLD_SIZE: start N ranks ourselves, as a CHILD
    process (torch.distributed.run), relay rank 0's JSON line, return its exit code."""
    import tempfile
    shared = tempfile.mkdtemp(prefix="lzs_bench_")
    port = free_port()
    env = dict(os.environ, LZS_BENCH_DIR=shared, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    print(f"bench.py: no WORLD_SIZE in the environment, launching {args.gpus} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    out_path = os.path.join(shared, "launch.stdout")
    import signal

    def end_group(proc, grace=5.0):
        # the group this call started, nothing else: SIGTERM first (the supervisors take their GPU workers along), then SIGKILL
        for sig, wait in ((signal.SIGTERM, grace), (signal.SIGKILL, None)):
            if proc.poll() is not None:
                break
            try:
                os.killpg(proc.pid, sig)
            except OSError:
                break
            try:
                proc.wait(timeout=wait)
            except subprocess.TimeoutExpired:
                pass

    class Ended(Exception):
        pass

    def on_signal(signum, _frame):
        raise Ended(signum)

    with open(out_path, "w+") as out:
        # A session of its own: on the deadline the whole group goes -- agent, supervisors and their workers.  That also
        # means a SIGTERM / SIGINT meant for THIS process (a `timeout 600 python bench.py`, the driver's own limit, Ctrl-C)
        # no longer reaches them by itself: take the group along on those too, and on any exception.
        proc = subprocess.Popen(cmd, env=env, stdout=out, start_new_session=True)
        old = {s: signal.signal(s, on_signal) for s in (signal.SIGTERM, signal.SIGINT, signal.SIGHUP)}
        try:
            rc = proc.wait(timeout=float(os.environ.get("LZS_BENCH_LAUNCH_DEADLINE", "3000")))
        except subprocess.TimeoutExpired:
            end_group(proc, grace=0.0)
            rc = 124
        except Ended as e:
            print(f"bench.py: signal {e.args[0]}: ending the ranks this call launched", file=sys.stderr, flush=True)
            end_group(proc)
            rc = 128 + int(e.args[0])
        except BaseException:
            end_group(proc)
            raise
        finally:
            for s, h in old.items():
                signal.signal(s, h)
        out.seek(0)
        text = out.read()
    if rc > 128:
        return rc
    line = last_json_line(text)
    if line is None:
        sys.stderr.write(text[-4000:])
        print("bench.py: the ranks produced no JSON line", file=sys.stderr)
        return rc or 1
    print(line, flush=True)
    return rc


def run_token() -> str:
    """Names the directory the supervisors of ONE launch meet in when the launcher did not give them one
    (the driver's torch.distributed.run): the parent agent's pid AND its start time (a later launch in the
    same pid namespace with the same port gets another directory, so no stale flag is ever read), the port,
    and torchelastic's run id."""
    ppid = os.getppid()
    try:
        start = open(f"/proc/{ppid}/stat").read().rsplit(")", 1)[1].split()[19]      # starttime, in clock ticks since boot
    except (OSError, IndexError):
        start = "0"
    rid = "".join(ch for ch in os.environ.get("TORCHELASTIC_RUN_ID", "") if ch.isalnum())[:16]
    return f"{ppid}_{start}_{os.environ.get('MASTER_PORT', '0')}_{rid or 'x'}"


def supervise(args, argv) -> int:
    """One of torch.distributed.run's ranks: run the RCCL job in a child process (so that a crash, a
    hang or an RCCL abort there leaves this process alive and clean of the GPU); if it fails on ANY
    rank, run the independent-shards fallback on EVERY rank.  Rank 0 relays the JSON line."""
    import signal
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    shared = os.environ.get("LZS_BENCH_DIR") or os.path.join("/tmp", "lzs_bench_" + run_token())
    os.makedirs(shared, exist_ok=True)
    current = {"proc": None}

    def on_term(signum, _frame):
        # torch.distributed.run ends the remaining ranks with SIGTERM when one exits non-zero: take the GPU
        # worker (this exact child) along instead of leaving it on the device
        proc = current["proc"]
        if proc is not None and proc.poll() is None:
            proc.kill()
            proc.wait()
        sys.exit(128 + signum)

    signal.signal(signal.SIGTERM, on_term)
    signal.signal(signal.SIGINT, on_term)
    env = dict(os.environ, LZS_BENCH_DIR=shared)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    worker_cmd = os.environ.get("LZS_BENCH_WORKER_CMD")          # tests: a stand-in worker
    cmd = (worker_cmd.split() if worker_cmd else [sys.executable, os.path.abspath(__file__)]) + list(argv)

    def flag(name: str, text: str = "") -> None:
        tmp = os.path.join(shared, f".{name}.tmp")
        with open(tmp, "w") as f:
            f.write(text)
        os.replace(tmp, os.path.join(shared, name))

    def flags(prefix: str):
        return [n for n in os.listdir(shared) if n.startswith(prefix)]

    def run_worker(role: str, deadline_s: float, watch_failures: bool):
        out_path = os.path.join(shared, f"out.{role}.{rank}")
        t_end = time.time() + deadline_s
        with open(out_path, "w+") as out:
            proc = subprocess.Popen(cmd, env=dict(env, LZS_BENCH_ROLE=role), stdout=out)
            current["proc"] = proc
            why, seen_fail_at = None, None
            while proc.poll() is None:
                time.sleep(0.2)
                if watch_failures and seen_fail_at is None and flags("fail1."):
                    seen_fail_at = time.time()
                if seen_fail_at is not None and time.time() - seen_fail_at > 5.0:
                    why = "another rank failed"
                elif time.time() > t_end:
                    why = f"no result after {deadline_s:.0f} s"
                if why:
                    proc.kill()                       # (this exact child)
                    proc.wait()
                    break
            out.seek(0)
            text = out.read()
        rc = proc.returncode
        return (rc if why is None else (rc or 1)), text, why

    line, reason = None, None
    ok = False
    if os.environ.get("LZS_BENCH_FORCE_FALLBACK"):
        reason = "LZS_BENCH_FORCE_FALLBACK is set"
    else:
        rc, text, why = run_worker("job", float(os.environ.get("LZS_BENCH_JOB_DEADLINE", "1500")), True)
        line = last_json_line(text)
        ok = rc == 0 and (rank != 0 or line is not None)
        if not ok:
            flag(f"fail1.{rank}", why or f"exit code {rc}")
            print(f"bench.py: rank {rank}: the sharded job failed ({why or f'exit code {rc}'})", file=sys.stderr, flush=True)
    # ---- agree on the outcome of the first attempt: every rank reports, any failure sends all to the fallback
    flag(f"done1.{rank}", "ok" if ok else "fail")
    t_end = time.time() + float(os.environ.get("LZS_BENCH_JOB_DEADLINE", "1500")) + 60
    while len(flags("done1.")) < world and time.time() < t_end:
        time.sleep(0.1)
    failed = sorted(flags("fail1."))
    everybody_ok = ok and not failed and len(flags("done1.")) == world
    if not everybody_ok:
        if reason is None:
            notes = []
            for n in failed[:3]:
                try:
                    notes.append(f"rank {n.split('.')[-1]}: {open(os.path.join(shared, n)).read().strip()}")
                except OSError:
                    pass
            reason = "the RCCL scatter / compress / gather job failed (" + "; ".join(notes or ["a rank did not report"]) + ")"
        flag("reason", reason)
        rc, text, why = run_worker("independent", float(os.environ.get("LZS_BENCH_FALLBACK_DEADLINE", "900")), False)
        line = last_json_line(text)
        ok = rc == 0 and (rank != 0 or line is not None)
        if not ok:
            print(f"bench.py: rank {rank}: the fallback failed too ({why or f'exit code {rc}'})", file=sys.stderr, flush=True)
            sys.stderr.write(text[-2000:])
    if rank == 0 and line is not None:
        print(line, flush=True)
    return 0 if ok else 1


# ============================================================================ workers (GPU)
def pick_device(args):
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    n = torch.cuda.device_count()
    if n == 0:
        raise SystemExit("bench.py: no GPU visible (there is no CPU path)")
    if local_rank >= n and not args.allow_shared_gpu:
        raise SystemExit(f"bench.py: LOCAL_RANK {local_rank} but only {n} GPU(s) visible (--allow-shared-gpu to share, for tests)")
    torch.cuda.set_device(local_rank % n)
    return torch.device("cuda", local_rank % n)


def hbm_needed(job_bytes: int, nb: int, cb: int, world: int, is_root: bool, slot_stride: int) -> int:
    """Everything a rank of the config-5 job holds in HBM: the job's own buffers (`job_bytes`:
    ShardedCompressJob.memory_needed), on the root also every rank's generated input, and the buffers of the
    checks after the timed region (slots, a fresh compaction, the decoded blocks), plus 2 GiB of headroom."""
    need = job_bytes + (world * nb * BLOCK if is_root else 0)
    return need + cb * (2 * slot_stride + BLOCK + slot_stride) + (2 << 30)


def check_ranges(lo: int, hi: int, check_every: int):
    """Which blocks of a chunk [lo, hi) the root compares with the CPU oracle: the first 1/check_every of
    them (one contiguous range of the gathered stream) and the last block; with check_every 1 all of them."""
    m = max(1, (hi - lo + check_every - 1) // max(1, check_every))
    return ((lo, lo + m), (hi - 1, hi)) if m < hi - lo else ((lo, hi),)


def job_callbacks(kernel_ev):
    """The two device operations the job is built around, as bench.py passes them to ShardedCompressJob."""
    cap = lzs.compressed_max(BLOCK)

    def compress(x, slots, lens):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        lzs.compress_blocks(x, None, cap, slots, lens)
        b.record()
        kernel_ev.append((a, b, x.shape[0]))

    def compact(slots, lens, dense, offsets):
        lzs.compact(slots, lens, dense=dense, offsets=offsets)

    return compress, compact


def run_sharded(args, dist, rank: int, world: int, dev) -> dict:
    """The config-5 job (lzs_compression_amd/sharded_job.py), K timed passes; returns the result on
    rank 0 (None elsewhere)."""
    from lzs_compression_amd.sharded_job import ShardedCompressJob
    nb = nb_asked = args.blocks if args.blocks is not None else 131072
    cap = lzs.compressed_max(BLOCK)
    slot_stride = (cap + 15) // 16 * 16
    # ---- a memory plan that degrades instead of failing: everything this rank will hold -- the job's buffers,
    # on the root also every rank's generated input, and the buffers of the checks after the timed region --
    # against the HBM that is free; while it does not fit on EVERY rank the shard is halved (and the line says so)
    while True:
        cb = nb if args.no_overlap else min(nb, args.chunk_blocks)
        need = hbm_needed(ShardedCompressJob.memory_needed(nb, BLOCK, slot_stride, world, cb, rank == 0), nb, cb, world, rank == 0, slot_stride)
        free, _total = torch.cuda.mem_get_info(dev)
        fits = torch.tensor([1 if free >= need else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(fits, op=dist.ReduceOp.MIN)
        if int(fits.item()) or nb <= 1024:
            break
        nb //= 2
    kernel_ev = []
    compress, compact = job_callbacks(kernel_ev)
    job = ShardedCompressJob(nb, BLOCK, slot_stride, dev, compress, compact, torch.cuda.synchronize, chunk_blocks=cb)
    # ---- the root generates every rank's blocks in HBM, one piece (<= 8 GiB) per rank
    pieces = None
    t_gen = time.perf_counter()
    if rank == 0:
        pieces = [workload.fill_device(args.workload, nb, BLOCK, first_block=r * nb, device=dev) for r in range(world)]
        torch.cuda.synchronize()
    t_gen = time.perf_counter() - t_gen

    def barrier():
        torch.cuda.synchronize()
        dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        job.step(pieces)
    kernel_ev.clear()
    barrier()
    t0 = time.perf_counter()
    steps = [job.step(pieces) for _ in range(args.steps)]
    barrier()
    elapsed = time.perf_counter() - t0
    kernel_ms = [a.elapsed_time(b) for a, b, _n in kernel_ev]
    kernel_blocks = [n for _a, _b, n in kernel_ev]
    stage_ms = job.last_stage_ms
    # ---- every phase alone: one un-overlapped pass (outside the timed region), same results
    serial = job.serial_phases(pieces)
    barrier()
    t = torch.tensor([elapsed, serial["scatter"], serial["compress"], serial["gather"], serial["total"],
                      float(np.mean([s["comm_busy"] for s in steps])), float(np.mean([s["compute_busy"] for s in steps]))],
                     dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed, sc, co, ga, tot, comm_busy, comp_busy = (float(v) for v in t.tolist())

    # ---- checks outside the timed region.  Every rank: chunk by chunk, compress again, decode on the device
    # (== the input) and compact again (== the bytes the job kept and sent)
    x = pieces[0] if rank == 0 else job.mine
    ok = True
    chk_slots = torch.empty((job.cb, slot_stride), dtype=torch.uint8, device=dev)
    chk_lens = torch.empty(job.cb, dtype=torch.int32, device=dev)
    chk_dense = torch.empty(job.cb * slot_stride, dtype=torch.uint8, device=dev)
    chk_off = torch.empty(job.cb + 1, dtype=torch.int64, device=dev)
    for j in range(job.K):
        lo, hi = job._chunk(j)
        n = hi - lo
        lzs.compress_blocks(x[lo:hi], None, cap, chk_slots[:n], chk_lens[:n])
        back, back_len = lzs.decompress_blocks(chk_slots[:n], chk_lens[:n], BLOCK)
        ok = ok and bool((back_len == BLOCK).all()) and torch.equal(back[:, :BLOCK], x[lo:hi])
        del back
        lzs.compact(chk_slots[:n], chk_lens[:n], dense=chk_dense, offsets=chk_off[:n + 1])
        cnt = int(chk_off[n].item())
        ok = ok and cnt == job.chunk_counts[j][rank] and torch.equal(chk_dense[:cnt], job._dense_chunk(j)[:cnt])
        ok = ok and torch.equal(chk_lens[:n], job.lens[lo:hi])
    del chk_slots, chk_dense
    okt = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
    dist.all_reduce(okt, op=dist.ReduceOp.MIN)
    lens_h = job.lens.cpu().numpy()
    result = None
    if rank == 0:
        # ... and the root compares its gathered bytes with the CPU oracle: of every chunk of every rank
        # the first 1/check_every blocks (one contiguous range of the gathered stream) and the last block
        import oracle
        O = oracle.oracle()
        cores = usable_cores()
        all_lens = job.all_lens.cpu().numpy().astype(np.int64)
        offs = np.concatenate([[0], np.cumsum(all_lens)])
        gathered_ok = int(offs[-1]) == sum(job.counts) == int(job.out.numel())
        compared = 0
        t_chk = time.perf_counter()
        for r in range(world):
            for j in range(job.K):
                lo, hi = job._chunk(j)
                for a, b in check_ranges(lo, hi, args.check_every):
                    rows = pieces[r][a:b].cpu().numpy()
                    want, want_len, _ = oracle.run_blocks(O, rows, threads=cores)
                    g0 = r * nb + a
                    got = job.out[int(offs[g0]):int(offs[g0 + (b - a)])].cpu().numpy()
                    gathered_ok = gathered_ok and bool((want_len == all_lens[g0:g0 + (b - a)]).all())
                    if gathered_ok:
                        cat = np.concatenate([want[i, :want_len[i]] for i in range(b - a)])
                        gathered_ok = cat.size == got.size and bool(np.array_equal(cat, got))
                    compared += b - a
        t_chk = time.perf_counter() - t_chk
        total_in = world * nb * BLOCK
        in_bytes = nb * BLOCK
        per_gib = [ms / (n * BLOCK / 2**30) for ms, n in zip(kernel_ms, kernel_blocks)]
        avg_ms_per_gib = float(np.mean(per_gib))
        achieved = 2**30 / (avg_ms_per_gib * 1e-3) / 1e9
        algo_bytes = in_bytes + int(lens_h.sum()) + 4 * nb
        result = {
            "metric": METRIC,
            "value": total_in * args.steps / elapsed / 1e9,
            "unit": "GB/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "config": {"workload": f"{world * nb} independent 64 KiB blocks ({world * nb * BLOCK / 2**30:g} GiB / {world} GPUs), class "
                                   f"'{args.workload}', generated in HBM on the root GPU, scattered {nb} blocks "
                                   f"({nb * BLOCK / 2**30:g} GiB) per rank over RCCL/xGMI, compressed, compacted, gathered to the root",
                       "class": args.workload, "blocks_per_gpu": nb, "block_bytes": BLOCK,
                       "sharding": f"contiguous block ranges, {nb} per rank; a step = the whole job: scatter || compress || gather, "
                                   f"pipelined over chunks of {job.cb} blocks" if job.overlap else
                                   f"contiguous block ranges, {nb} per rank; a step = scatter, then compress, then gather",
                       "compression_ratio": float(all_lens.sum()) / total_in,
                       "blocks_per_gpu_asked": nb_asked,
                       "memory_plan": "as asked" if nb == nb_asked else f"shard halved to {nb} blocks per GPU: the HBM free on some rank did not hold {nb_asked}"},
            "overlap": bool(job.overlap), "chunk_blocks": job.cb, "chunks_per_rank": job.K,
            "end_to_end_GBps": total_in * args.steps / elapsed / 1e9,
            "phases_ms": {"scatter": sc * 1e3, "compress": co * 1e3, "gather": ga * 1e3, "step": tot * 1e3,
                          "note": "each phase ALONE: one un-overlapped pass of the same job after the timed steps, every phase "
                                  "ended by a device synchronize, MAX over ranks; compress includes the compaction of the slots"},
            "serial_end_to_end_GBps": total_in / tot / 1e9,
            "compute_only_GBps": total_in / co / 1e9,
            "scatter_GBps": (world - 1) * nb * BLOCK / sc / 1e9 if sc > 0 and world > 1 else None,
            "gather_GBps": (sum(job.counts) - job.counts[0]) / ga / 1e9 if ga > 0 and world > 1 else None,
            # per xGMI link of the root: its N - 1 peers are served at once, one link each (DESIGN.md section 6 assumes
            # 45-60 GB/s a link; point to point, 7 links x ~153 GB/s per GPU)
            "scatter_GBps_per_link": nb * BLOCK / sc / 1e9 if sc > 0 and world > 1 else None,
            "gather_GBps_per_link": (sum(job.counts) - job.counts[0]) / (world - 1) / ga / 1e9 if ga > 0 and world > 1 else None,
            "overlapped_step": {"comm_busy_ms": comm_busy * 1e3, "compute_busy_ms": comp_busy * 1e3,
                                "stage_comm_ms_rank0_last_step": stage_ms.get("comm"), "stage_compute_ms_rank0_last_step": stage_ms.get("compute"),
                                "note": "HIP events around every stage's batch of point-to-point operations (comm) and every "
                                        "chunk's compress + compact (compute); busy = their sums, mean over steps, MAX over ranks"},
            "gathered_bytes": int(sum(job.counts)),
            "generate_on_root_s": t_gen,
            "checks": {"every_rank_round_trip_on_device": bool(okt.item()), "gathered_samples_equal_oracle": bool(gathered_ok),
                       "gathered_blocks_compared_with_oracle": compared, "of": world * nb, "oracle_check_s": t_chk},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": None,
                         "kernel": "lzs_compress_blocks_wg_kernel (rank 0's launches, beside the RCCL transfers)",
                         "algorithmic_bytes_per_GiB_launch": {"read_input": 2**30, "total_read_plus_written": algo_bytes * 2**30 // in_bytes},
                         "avg_kernel_ms_per_GiB": avg_ms_per_gib, "launches": len(kernel_ms)},
        }
        if not args.no_cpu_baseline:
            # the host codec on a bounded sample of rank 0's blocks, after the timed region (north_star: the
            # 1/2/4/8 figures next to the reference C path timed on the same box's host cores)
            result["cpu_baseline"], _o, _l = cpu_sample(pieces[0][:min(nb, 4096)].cpu().numpy())
    dist.barrier()
    return result


def worker_job(args) -> int:
    """Role "job": one rank of the RCCL job (child of a supervisor, or the process itself at world 1)."""
    import datetime
    heavy_imports()
    import torch.distributed as dist
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29531")
    dev = pick_device(args)
    # a collective that does not complete in 5 minutes aborts the process: the supervisor falls back
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev, timeout=datetime.timedelta(seconds=300))
    result = run_sharded(args, dist, rank, world, dev)
    dist.destroy_process_group()
    if rank == 0:
        emit(result)
    return 0


def worker_independent(args) -> int:
    """Role "independent" (the fallback): every rank compresses a shard of its own, generated on its own
    GPU; NO collective, no RCCL -- ranks meet at a barrier made of files.  The compute-only
    weak-scaling figure of round 1, labelled as a fallback."""
    heavy_imports()
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    shared = os.environ["LZS_BENCH_DIR"]
    dev = pick_device(args)
    nb = args.blocks if args.blocks is not None else 131072
    cap = lzs.compressed_max(BLOCK)
    slot_stride = (cap + 15) // 16 * 16
    x = workload.fill_device(args.workload, nb, BLOCK, first_block=rank * nb, device=dev)
    slots = torch.empty((nb, slot_stride), dtype=torch.uint8, device=dev)
    lens = torch.empty(nb, dtype=torch.int32, device=dev)

    def file_barrier(name: str, timeout: float = 600.0) -> None:
        open(os.path.join(shared, f"{name}.{rank}"), "w").close()
        t_end = time.time() + timeout
        while True:
            have = sum(1 for n in os.listdir(shared) if n.startswith(name + "."))
            if have >= world:
                return
            if time.time() > t_end:
                raise SystemExit(f"bench.py: rank {rank}: {have} of {world} ranks reached '{name}'")
            time.sleep(0.0005)

    for _ in range(args.warmup):
        lzs.compress_blocks(x, None, cap, slots, lens)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    torch.cuda.synchronize()
    file_barrier("ready2")
    t0 = time.perf_counter()
    for k in range(args.steps):
        ev[k][0].record()
        lzs.compress_blocks(x, None, cap, slots, lens)
        ev[k][1].record()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    kernel_ms = [a.elapsed_time(b) for a, b in ev]
    back, back_len = lzs.decompress_blocks(slots, lens, BLOCK)
    ok = bool((back_len == BLOCK).all()) and torch.equal(back[:, :BLOCK], x)
    del back
    # sampled blocks against the CPU oracle (first, middle, last 64 of the shard)
    import oracle
    O = oracle.oracle()
    exact = True
    for a in sorted({0, max(0, nb // 2 - 32), max(0, nb - 64)}):
        b = min(nb, a + 64)
        want, want_len, _ = oracle.run_blocks(O, x[a:b].cpu().numpy(), threads=2)
        g, gl = slots[a:b].cpu().numpy(), lens[a:b].cpu().numpy()
        exact = exact and bool((want_len == gl).all()) and all(
            np.array_equal(g[i, :gl[i]], want[i, :want_len[i]]) for i in range(b - a))
    mine = {"rank": rank, "elapsed": elapsed, "kernel_ms": kernel_ms, "bytes_out": int(lens.sum().item()), "round_trip": ok, "oracle": exact}
    tmp = os.path.join(shared, f".res2.{rank}.tmp")
    json.dump(mine, open(tmp, "w"))
    os.replace(tmp, os.path.join(shared, f"res2.{rank}"))
    if rank != 0:
        return 0
    t_end = time.time() + 600
    while sum(1 for n in os.listdir(shared) if n.startswith("res2.")) < world:
        if time.time() > t_end:
            raise SystemExit("bench.py: not every rank delivered its fallback result")
        time.sleep(0.01)
    res = [json.load(open(os.path.join(shared, f"res2.{r}"))) for r in range(world)]
    elapsed = max(r["elapsed"] for r in res)
    total_in = world * nb * BLOCK
    try:
        reason = open(os.path.join(shared, "reason")).read().strip()
    except OSError:
        reason = "unknown"
    avg_ms = float(np.mean(kernel_ms))
    achieved = nb * BLOCK / (avg_ms * 1e-3) / 1e9
    base = None
    if not args.no_cpu_baseline:
        base, _o, _l = cpu_sample(x[:min(nb, 4096)].cpu().numpy())
    emit({
        # NOT the contract's number: `value` stays empty so that nobody reads a compute-only figure as the
        # end-to-end rate of config 5; the measurement is in compute_only_GBps
        "metric": METRIC, "value": None, "unit": "GB/s", "n_gpus": world, "valid": False,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
        "config": {"workload": f"FALLBACK: {world * nb} independent 64 KiB blocks, class '{args.workload}', {nb} per GPU generated on "
                               f"that GPU, compressed there; NO scatter / gather (the RCCL job did not complete)",
                   "class": args.workload, "blocks_per_gpu": nb, "block_bytes": BLOCK,
                   "sharding": "independent shards, no data-path collective, ranks synchronised through files",
                   "compression_ratio": sum(r["bytes_out"] for r in res) / total_in},
        "fallback": {"reason": reason, "what": "compute-only weak scaling (compute_only_GBps); `value` is empty because this is NOT "
                                                 "the end-to-end rate of config 5"},
        "compute_only_GBps": total_in * args.steps / elapsed / 1e9,
        "cpu_baseline": base,
        "per_rank_elapsed_s": [r["elapsed"] for r in res],
        "checks": {"every_rank_round_trip_on_device": all(r["round_trip"] for r in res),
                   "sampled_blocks_equal_oracle": all(r["oracle"] for r in res)},
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                     "traffic": None, "kernel": "lzs_compress_blocks_wg_kernel (rank 0's launches)",
                     "algorithmic_bytes_per_launch": {"read_input": nb * BLOCK}, "avg_kernel_ms": avg_ms},
    })
    return 0


def config5_world1(args, dev) -> dict:
    """N = 1 only, after the headline: the config-5 job at world size 1 on the nccl backend (no peers:
    the scatter and the gather move nothing over xGMI), 8 GiB in chunks -- the same fields the N > 1
    lines carry, so the scaling curve's first point can be read on the same basis."""
    import datetime
    import torch.distributed as dist
    # a rendezvous of its own (not env://: under torch.distributed.run the environment points at the
    # agent's store, and this process is not one of ITS ranks' workers in the N > 1 sense)
    agent_store = os.environ.pop("TORCHELASTIC_USE_AGENT_STORE", None)      # (else c10d would look for the agent's store at OUR port)
    try:
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{free_port()}", rank=0, world_size=1, device_id=dev,
                                timeout=datetime.timedelta(seconds=120))
    finally:
        if agent_store is not None:
            os.environ["TORCHELASTIC_USE_AGENT_STORE"] = agent_store
    try:
        sub = argparse.Namespace(**vars(args))
        sub.blocks = 131072 if args.blocks in (None, 16384) else args.blocks
        sub.steps, sub.warmup = min(args.steps, 3), 1
        sub.no_cpu_baseline = True                    # (the N = 1 line carries it already)
        r = run_sharded(sub, dist, 0, 1, dev)
    finally:
        dist.destroy_process_group()
    keep = ("value", "ms_per_step", "steps", "overlap", "chunk_blocks", "chunks_per_rank", "end_to_end_GBps", "phases_ms",
            "serial_end_to_end_GBps", "compute_only_GBps", "overlapped_step", "gathered_bytes", "checks")
    out = {k: r[k] for k in keep}
    out["workload"] = r["config"]["workload"]
    return out


def block_decoder(x, slots, lens, launches: int = 5) -> dict:
    """The way back, beside the headline (not part of `value`): lzs_decompress_batch_device on the slots the timed launches
    left in HBM, `launches` launches between HIP events on the launch stream after 2 warm-ups, every byte compared with
    the input."""
    try:
        nb = x.shape[0]
        back, back_len = lzs.decompress_blocks(slots, lens, BLOCK)
        lzs.decompress_blocks(slots, lens, BLOCK, back, back_len)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        torch.cuda.synchronize()
        for a, b in ev:
            a.record()
            lzs.decompress_blocks(slots, lens, BLOCK, back, back_len)
            b.record()
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in ev]
        ok = bool((back_len == BLOCK).all()) and torch.equal(back[:, :BLOCK], x)
        del back
        return {"entry": "lzs_decompress_batch_device", "kernel": "lzs_decompress_blocks_grp_kernel", "launches": launches,
                "avg_kernel_ms": float(np.mean(ms)), "min_kernel_ms": float(np.min(ms)),
                "value": nb * BLOCK / (float(np.mean(ms)) * 1e-3) / 1e9, "unit": "GB/s of output", "round_trip": ok}
    except Exception as exc:                          # noqa: BLE001 -- an extra, never the contract line's problem
        return {"error": str(exc)}


def other_class(cls: str, nb: int, dev, launches: int = 10) -> dict:
    """One more 1 GiB class on the driver's line (BASELINE.json configs[2] low entropy, configs[3] high
    entropy), measured like the headline: seeded blocks into HBM, 2 warm-up launches, `launches`
    launches between HIP events on the launch stream, then EVERY block against the host codec."""
    host = workload.fill(cls, nb, BLOCK, first_block=0)
    x = torch.from_numpy(host).to(dev)
    cap = lzs.compressed_max(BLOCK)
    slot_stride = (cap + 15) // 16 * 16
    slots = torch.empty((nb, slot_stride), dtype=torch.uint8, device=dev)
    lens = torch.empty(nb, dtype=torch.int32, device=dev)
    for _ in range(2):
        lzs.compress_blocks(x, None, cap, slots, lens)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for a, b in ev:
        a.record()
        lzs.compress_blocks(x, None, cap, slots, lens)
        b.record()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    kernel_ms = [a.elapsed_time(b) for a, b in ev]
    lens_h = lens.cpu().numpy()
    avg_ms = float(np.mean(kernel_ms))
    in_bytes = nb * BLOCK
    achieved = in_bytes / (avg_ms * 1e-3) / 1e9
    decoder = block_decoder(x, slots, lens)
    limiter, limiter_note = pmc_limiter(cls) if nb == 16384 else (None, "the counters were taken at 16384 blocks per launch")
    traffic, traffic_note = pmc_traffic(cls) if nb == 16384 else (None, "the counters were taken at 16384 blocks per launch")
    return {"workload": f"{nb} independent 64 KiB blocks ({nb * BLOCK >> 20} MiB), class '{cls}' (seeded generator), device-resident",
            "value": in_bytes * launches / elapsed / 1e9, "unit": "GB/s", "launches": launches,
            "ms_per_step": elapsed / launches * 1e3, "avg_kernel_ms": avg_ms, "min_kernel_ms": float(np.min(kernel_ms)),
            "compression_ratio": float(lens_h.sum()) / in_bytes,
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "traffic": (traffic or {}).get("hbm_bytes"),
                         "algorithmic_bytes_per_launch": {"read_input": in_bytes, "total_read_plus_written": in_bytes + int(lens_h.sum()) + 4 * nb},
                         "limiter": limiter if limiter else limiter_note},
            "block_decoder": decoder,
            "check": check_every_block(host, lens_h, slots)}


def single(args) -> int:
    """N = 1: BASELINE.json configs[1], in this process."""
    heavy_imports()
    dev = pick_device(args)
    if args.sharded_job:
        os.environ["WORLD_SIZE"], os.environ["RANK"] = "1", "0"
        return worker_job(args)
    nb = args.blocks if args.blocks is not None else 16384

    # ---- the blocks of the seeded class, into HBM
    host = workload.fill(args.workload, nb, BLOCK, first_block=0)
    x = torch.from_numpy(host).to(dev)
    slot_stride = (lzs.compressed_max(BLOCK) + 15) // 16 * 16
    slots = torch.empty((nb, slot_stride), dtype=torch.uint8, device=dev)
    lens = torch.empty(nb, dtype=torch.int32, device=dev)
    cap = lzs.compressed_max(BLOCK)

    def step():
        lzs.compress_blocks(x, None, cap, slots, lens)

    def barrier():                   # (N = 1: no other rank to wait for)
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    # per-launch durations with HIP events on the stream the kernel is launched on
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(args.steps)]
    barrier()
    t0 = time.perf_counter()
    for k in range(args.steps):
        ev[k][0].record()
        step()
        ev[k][1].record()
    barrier()
    elapsed = time.perf_counter() - t0
    kernel_ms = [a.elapsed_time(b) for a, b in ev]

    total_in = nb * BLOCK * args.steps
    lens_h = lens.cpu().numpy()
    ratio = float(lens_h.sum()) / (nb * BLOCK)

    avg_ms = float(np.mean(kernel_ms))
    traffic, traffic_note = pmc_traffic(args.workload) if nb == 16384 else (None, "the counters were taken at 16384 blocks per launch")
    in_bytes = nb * BLOCK
    algo_bytes = in_bytes + int(lens_h.sum()) + 4 * nb
    achieved = in_bytes / (avg_ms * 1e-3) / 1e9
    result = {
        "metric": METRIC,
        "value": total_in / elapsed / 1e9,
        "unit": "GB/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic",
        "config": {"workload": f"{nb} independent 64 KiB blocks per GPU ({nb * BLOCK >> 20} MiB), "
                               f"class '{args.workload}' (seeded generator), device-resident",
                   "class": args.workload, "blocks_per_gpu": nb, "block_bytes": BLOCK,
                   "sharding": "one GPU, no data-path collective",
                   "compression_ratio": ratio},
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS,
                     "traffic": (traffic or {}).get("hbm_bytes"), "traffic_detail": traffic if traffic else traffic_note,
                     "kernel": "lzs_compress_blocks_wg_kernel",
                     "kernel_note": "one launch = lzs_classify_blocks_kernel + the kernel's variant for each class of block over the same "
                                    "grid (wgv_text the default at six workgroups per CU, wgv_few and wgv_lit without a 3-byte chain at eight; "
                                    "a workgroup whose block is another variant's returns at once): the events bracket all of them",
                     "algorithmic_bytes_per_launch": {"read_input": in_bytes,
                                                      "total_read_plus_written": algo_bytes},
                     "avg_kernel_ms": avg_ms, "min_kernel_ms": float(np.min(kernel_ms)),
                     "median_kernel_ms": float(np.median(kernel_ms)),
                     "total_GBps": algo_bytes / (avg_ms * 1e-3) / 1e9},
    }
    limiter, limiter_note = pmc_limiter(args.workload) if nb == 16384 else (None, "the counters were taken at 16384 blocks per launch")
    result["roofline"]["limiter"] = limiter if limiter else limiter_note
    if args.dump_outputs:
        info = dump_outputs(args.dump_outputs, slots, lens)
        print(f"bench.py: wrote {', '.join(info['files'])} ({info['bytes']} bytes) to {info['dir']}", file=sys.stderr, flush=True)
    if args.full:
        # the buffers are handed over, so that full_extras can free them before the other classes are set up
        bufs = [host, x, slots, lens]
        del host, x, slots, lens
        full_extras(args, dev, result, bufs, lens_h, nb, achieved, avg_ms, ratio)
    emit(result)
    return 0


def full_extras(args, dev, result, bufs, lens_h, nb, achieved, avg_ms, ratio) -> None:
    """--full, N = 1: everything the line carries beside the headline, each piece measured after the timed steps.
    `bufs` = [host blocks, device blocks, slots, lengths] of the headline launch; emptied here."""
    host, x, slots, lens = bufs
    bufs.clear()
    # the box's own streaming figure next to the 8 TB/s of the data sheet (report
    # the fraction against both): a device-to-device copy of the same 1 GiB, read + written
    try:
        y = torch.empty_like(x)
        for _ in range(2):
            y.copy_(x)
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0.record()
        for _ in range(10):
            y.copy_(x)
        c1.record()
        torch.cuda.synchronize()
        copy_gbps = 2.0 * x.numel() * 10 / (c0.elapsed_time(c1) * 1e-3) / 1e9
        del y
        result["roofline"]["measured_device_copy_GBps"] = copy_gbps
        result["roofline"]["frac_of_measured_copy"] = result["roofline"]["total_GBps"] / copy_gbps
        result["roofline"]["measured_copy_note"] = ("torch device-to-device copy of the input tensor, bytes read + written per second; "
                                                     "frac_of_measured_copy = the kernel's read + written bytes per second over it")
    except Exception as exc:                       # noqa: BLE001
        result["roofline"]["measured_device_copy_GBps"] = None
        result["roofline"]["measured_copy_note"] = f"copy measurement failed: {exc}"
    result["block_decoder"] = block_decoder(x, slots, lens)
    if not args.no_single_stream:
        # secondary, outside the timed region: the same bytes as ONE stream through
        # lzs_compress_stream_device, wall clock around the synchronous call
        try:
            flat = x.reshape(-1)
            buf, nbytes = lzs.compress_stream(flat)
            t = time.perf_counter()
            buf, nbytes = lzs.compress_stream(flat, buf)
            dt = time.perf_counter() - t
            result["single_stream"] = {"entry": "lzs_compress_stream_device", "input_bytes": int(flat.numel()),
                                       "compressed_bytes": nbytes, "ms": dt * 1e3,
                                       "value": flat.numel() / dt / 1e9, "unit": "GB/s"}
            back, got = lzs.decompress_stream(buf[:nbytes], flat.numel() + 16)
            t = time.perf_counter()
            back, got = lzs.decompress_stream(buf[:nbytes], flat.numel() + 16, back)
            dt = time.perf_counter() - t
            result["single_stream"]["decompress"] = {
                "entry": "lzs_decompress_stream_device", "ms": dt * 1e3, "value": got / dt / 1e9,
                "unit": "GB/s of output", "round_trip": bool(got == flat.numel() and torch.equal(back[:got], flat))}
            del buf, back
        except Exception as exc:                      # never let the extra line spoil the contract line
            result["single_stream"] = {"error": str(exc)}
    if not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline(host, lens_h, slots)
    del slots, x, host, lens
    if not args.no_other_classes:
        # BASELINE.json configs[2] and [3] (or whichever two classes the headline is not), same launch, same check
        result["other_classes"] = {}
        for cls in CLASS_NAMES:
            if cls != args.workload:
                try:
                    result["other_classes"][cls] = other_class(cls, nb, dev)
                except Exception as exc:                  # noqa: BLE001 -- an extra, never the contract line's problem
                    result["other_classes"][cls] = {"error": f"{type(exc).__name__}: {exc}"}
    # All three classes where the driver parses them: BASELINE.json configs[1..3] as first-class numbers
    # inside `roofline`, each measured like the headline and checked block by block.
    by_class = {args.workload: {"GBps": achieved, "frac": achieved / HBM_PEAK_GBS, "kernel_ms": avg_ms, "ratio": ratio,
                                "checked_blocks": ((result.get("cpu_baseline") or {}).get("check") or {}).get("blocks_compared"),
                                "bit_exact": ((result.get("cpu_baseline") or {}).get("check") or {}).get("bit_exact")}}
    for cls, r in (result.get("other_classes") or {}).items():
        if "error" in r:
            by_class[cls] = {"error": r["error"]}
        else:
            by_class[cls] = {"GBps": r["roofline"]["achieved"], "frac": r["roofline"]["frac"], "kernel_ms": r["avg_kernel_ms"],
                             "ratio": r["compression_ratio"], "checked_blocks": r["check"]["blocks_compared"], "bit_exact": r["check"]["bit_exact"]}
    result["roofline"]["by_class"] = by_class
    if not args.no_config5:
        try:
            result["config5_world1"] = config5_world1(args, dev)
        except Exception as exc:                      # noqa: BLE001 -- an extra, never the contract line's problem
            result["config5_world1"] = {"error": f"{type(exc).__name__}: {exc}"}


def main() -> int:
    argv = sys.argv[1:]
    args = parse_args(argv)
    if args.dump_outputs and (args.gpus > 1 or args.sharded_job):
        raise SystemExit("bench.py: --dump-outputs writes the outputs of the N = 1 launch only")
    role = os.environ.get("LZS_BENCH_ROLE")
    if role == "job":
        return worker_job(args)
    if role == "independent":
        return worker_independent(args)
    world = int(os.environ.get("WORLD_SIZE", "0") or 0)
    # (LZS_BENCH_FORCE_SUPERVISE: tests run the supervisor -> worker -> RCCL rendezvous chain with one rank on a one-GPU box)
    if world > 1 or (world == 1 and os.environ.get("LZS_BENCH_FORCE_SUPERVISE")):
        if world != args.gpus:
            raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
        return supervise(args, argv)
    if args.gpus > 1:
        return self_launch(args, argv)
    return single(args)


if __name__ == "__main__":
    sys.exit(main())
