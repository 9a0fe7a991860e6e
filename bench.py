#!/usr/bin/env python3
"""bench.py -- IQ Msamples/s through demod + xcorr on MI355X (BASELINE.json metric).

A step = one pass of the hot path (u8 IQ -> FM discriminator -> FFT -> conj-multiply -> inverse FFT -> peak pick)
over one synthetic capture set already resident in HBM; peaks end on the host.

  --config cfg2 (default)              3 stations x 2 Msps x 100 s, 99 windows x 3 pairs, L = 2 000 000, N = 2^21
  --config cfg3                        weak_signal_simulator.go captures, 10 s windows (L = 2e7, N = 5 x 2^22; TDOA_POW2_ONLY=1: 2^25), 342 windows
                                       x 3 pairs = 1026 pair-windows streamed in launch groups
  --config cfg4                        8 stations (28 pairs) x 2 Msps x 100 s
  --config cfg5                        16 stations (120 pairs) x 4 Msps x 300 s, 1 s windows (L = 4e6, N = 2^22)

Multi-GPU (one rank per GPU, torch.distributed over RCCL; no collective on the data path):
  --scaling weak (default): one job of N x (the config's windows), window-major -- rank r holds and processes capture
      set r, ONE all-gather of the per-pair peak records per step, rank 0 decodes all of them and solves every set -- all
      inside the timed region.  Per-GPU work is fixed; value = the station-samples all ranks processed / time.
  --scaling strong (BASELINE config 4 as written: `--config cfg4 --scaling strong`): ONE capture set; rank r runs
      tdoa_process(ctx, r, world) on the windows it owns (wid % world == r), one all-gather, byte-wise owner merge and the
      N-station least-squares solve on rank 0 -- all inside the timed region.  value = the job's station-samples / time.
  At N > 1 the default run (cfg2, weak) with --full times BOTH: its contract line is the weak-scaled cfg2 job, and the
  sharded cfg4 job is timed right after it in the same process group and attached as `sharded_cfg4`.
  Multi-rank jobs correlate captures with TRUE delays (--sim fmdelay: one frequency-modulated carrier from TX, every
  station's copy delayed by its propagation time), so the solve inside the timed region has a position to find: the run
  FAILS unless every pair's median target-block lag equals the geometry's and the fix lies within 150 m of TX.

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line.  --full also reports what the
headline figure does not need: the roofline and per-kernel fields, the graph-replay leg, clocks and the sustained replay,
the end-to-end leg from host buffers, the CPU baseline with the window-0 parity check against the oracle and, at N > 1, the
sharded cfg4 job.  The --no-* switches below turn single legs of --full off.

Prints ONE JSON line on rank 0 (see the contract in the task description).
"""
import argparse
import hashlib
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "tdoa-geolocation_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# lat-lon-table.csv rows of the three collectors + simulator.go:229 example transmitter
STATIONS = [
    (41.18660274289527, -95.96064116595667, 355.69),   # kx0u
    (41.24669616513154, -96.08366304481238, 329.0),    # n3pay
    (41.32916620016985, -96.03513381562004, 373.18),   # kf0mtl
]
TX = (41.20, -96.00, 400.0)
SEED_BASE = 0x5D0A0000
HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: 8 TB/s spec (6.29 TB/s measured achievable)
HBM_FILL_GBS = 5800.0       # what a plain fill / out-of-place add sustains on the pool's boxes (profiles/r03_hbm_microbench.txt)

CONFIGS = {
    "cfg2": dict(stations=3, fs=2e6, block=66_666_666, wlen=2_000_000, sim="simulator", steps=10,
                 label="BASELINE config 2: 3 stations x 2 Msps x 100 s simulator.go-style capture"),
    "cfg3": dict(stations=3, fs=2e6, block=114 * 20_000_000, wlen=20_000_000, sim="weak", steps=3,
                 label="BASELINE config 3: weak_signal_simulator.go captures, 10 s windows, 1026 pair-windows"),
    "cfg4": dict(stations=8, fs=2e6, block=66_666_666, wlen=2_000_000, sim="simulator", steps=5,
                 label="BASELINE config 4: 8 collectors (28 pairs) x 2 Msps x 100 s"),
    "cfg5": dict(stations=16, fs=4e6, block=400_000_000, wlen=4_000_000, sim="simulator", steps=3,
                 label="BASELINE config 5: 16 collectors (120 pairs) x 4 Msps x 300 s, 1 s windows"),
}


class BenchCheckFailed(Exception):
    """a check after a job's timed region failed on this rank; main() makes every rank of the group agree on it (one
    all-reduce) so that nobody is left waiting in a collective for a rank that has gone"""


def station_table(n):
    """the 3 real collectors + synthetic ones on 12 / 7 km rings about their centroid"""
    out = list(STATIONS)
    clat = sum(s[0] for s in STATIONS) / 3
    clon = sum(s[1] for s in STATIONS) / 3
    k = 0
    while len(out) < n:
        ang = 2 * math.pi * (k + 0.37) / max(n - 3, 1)
        r_km = 12.0 if k % 2 == 0 else 7.0
        out.append((clat + r_km / 111.2 * math.cos(ang), clon + r_km / (111.2 * math.cos(math.radians(clat))) * math.sin(ang),
                    300.0 + 10.0 * k))
        k += 1
    return out


HOT_SOURCES = ("device_common.hpp", "k1_discriminator.hpp", "k1_single_look.hpp", "fft_stockham.hpp", "fft_radix16.hpp",
               "fft_radix8.hpp", "dec_stream.hpp", "dec_staged.hpp", "tdoa_mi355x.hip")


def source_hash():
    """hash of the sources of the timed path's kernels and their launch code: a committed PMC traffic file is only
    quoted when it was taken on these kernels"""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "tdoa-geolocation_amd", "csrc")
    for f in HOT_SOURCES:
        h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def _latest_profile(pattern):
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)))
    return files[-1] if files else None


def pmc_traffic(cfg_name, kernels):
    """HBM-side bytes per launch from the committed rocprofv3 --pmc passes of THIS configuration (scripts/collect_pmc.sh
    <tag> <cfg>); bench.py cannot profile itself, so this is read back from profiles/ -- and only if the file was taken on
    the current kernel sources.  `kernels`: the kernel names one profiling scope of the library covers.
    returns (bytes per launch summed over `kernels`, source label, sum over the step's kernels)"""
    f = _latest_profile("*pmc_traffic_%s.json" % cfg_name)
    if not f:
        return None, None, None
    try:
        doc = json.load(open(f))
        if doc.get("source_sha16") != source_hash():
            return None, "stale: %s was taken on other kernel sources" % os.path.basename(f), None
        recs = [doc["kernels"].get(k) for k in kernels]
        total = sum(v.get("traffic_bytes_per_step", v["traffic_bytes_per_launch"]) for v in doc["kernels"].values())      # one step
        mine = sum(r["traffic_bytes_per_launch"] for r in recs if r) if any(recs) else None
        return mine, os.path.basename(f), total
    except Exception:
        return None, None, None


N_SIMD, N_SE = 1024, 32          # MI355X: 256 CUs x 4 SIMDs; 8 XCDs x 4 shader engines


def sq_issue(cfg_name, kernel):
    """vector-instruction issue share of a kernel from the committed SQ counter table of THIS configuration (scripts/collect_sq.sh):
    SQ_ACTIVE_INST_VALU counts quad-cycles summed over the SIMDs, SQ_BUSY_CYCLES cycles summed over the shader engines
    (MI355X_MICROARCH.md, SQ PMC units).  None unless the table was taken on the current kernel sources."""
    f = _latest_profile("*sq_%s.csv" % cfg_name)
    if not f:
        return None
    try:
        lines = open(f).read().strip().splitlines()
        if not lines[0].startswith("# source_sha16=") or lines[0].split("=", 1)[1].strip() != source_hash():
            return None
        import csv
        for r in csv.DictReader(lines[1:]):
            if r["kernel"].split("<")[0] == kernel:
                valu, busy, waves = float(r["SQ_ACTIVE_INST_VALU"]), float(r["SQ_BUSY_CYCLES"]), float(r["SQ_WAVES"])
                lds, conf = float(r.get("SQ_LDS_IDX_ACTIVE", "nan")), float(r.get("SQ_LDS_BANK_CONFLICT", "nan"))
                return {"valu_issue_frac": round(valu * 4.0 / N_SIMD / (busy / N_SE), 3),
                        "valu_instructions_per_wave": round(float(r["SQ_INSTS_VALU"]) / waves, 1),
                        "lds_conflict_frac": None if not lds or lds != lds else round(conf / lds, 3),
                        "source": os.path.basename(f)}
    except Exception:
        pass
    return None


def path_switches():
    """TDOA_* environment switches that make the library take another path than its default (A/B runs): the committed counter
    files describe the default path's kernels and are not quoted next to them"""
    return sorted(k for k, v in os.environ.items() if k.startswith("TDOA_") and k not in ("TDOA_BENCH_BACKEND", "TDOA_LIB_VARIANT",
                                                                                          "TDOA_UPLOAD_THREADS") and v not in ("", "0"))


def decimation_fits(nc, max_lag):
    """the library's rule (tdoa_mi355x.hip decimation_design): a Kaiser filter of at most 95 taps a side must reach 120 dB
    between the pass band |m| <= M = max_lag/2 + 2 and the stop band |m| >= Nc/16 - M"""
    m, r = max_lag // 2 + 2, nc // 16
    if r - 2 * m <= 0:
        return False
    dw = 2.0 * math.pi * (r - 2 * m) / nc
    t = min(95, math.ceil((140.0 - 8.0) / (2.285 * dw) / 2.0))
    return 8.0 + 2.285 * dw * 2.0 * t >= 120.0


def cpu_info():
    model, phys = "unknown", set()
    try:
        pid = cid = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name") and model == "unknown":
                model = line.split(":", 1)[1].strip()
            elif line.startswith("physical id"):
                pid = line.split(":", 1)[1].strip()
            elif line.startswith("core id"):
                cid = line.split(":", 1)[1].strip()
            elif not line.strip():
                if pid is not None and cid is not None:
                    phys.add((pid, cid))
                pid = cid = None
    except OSError:
        pass
    return model, (len(phys) or (os.cpu_count() or 1))


def _mode_b_f64_unit(args):
    """one (pair, window) of the north-star pipeline in float64 on the CPU (worker process of the CPU-fft leg)"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import numpy as np
    from oracle import float_pipeline as fp
    a, b, max_lag = args
    lag, corr, _ = fp.xcorr_peak_u8(np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8), max_lag)
    return lag, corr


def cpu_baseline_leg(ctx, peaks, block, wlen, max_lag, budget_s):
    """BASELINE.md section 2.  Times the CPU oracle (restatement of processor.go crossCorrelate) on the host on a
    bounded sample of the same bytes, in the reference's own call pattern (3 pairs x {reference, target} block,
    processor.go:816-850): once on ONE thread (the reference is single-threaded), once with OpenMP on every core; the
    same algorithm as the GPU path in float64 on the CPU cores; and checks the GPU peaks of window 0 against the
    oracle.  This is the only place bench.py touches oracle/."""
    import ctypes
    from oracle import pyoracle as o
    o.build()
    model, phys = cpu_info()
    threads = os.cpu_count() or 1
    # --- parity of the timed GPU path on window 0 (mode B oracle, f64 FFT form); 10 s windows are left to the tests
    parity = None
    if wlen <= 4_000_000:
        w0 = [ctx.capture_download(s, 0, wlen) for s in range(3)]
        pre = [o.b_preprocess(x)[0] for x in w0]
        parity = True
        for p, (i, j) in enumerate([(0, 1), (0, 2)]):             # pairs (0,1), (0,2) are slots 0, 1 for any station count
            olag, ocorr, _ = o.b_xcorr_peak_fft(pre[i], pre[j], max_lag)
            g = peaks[0, p]
            if int(g["lag"]) != olag or abs(float(g["corr"]) - ocorr) > 1e-5 * max(abs(ocorr), 1e-30):
                parity = False
    # --- the reference's call pattern on the first n samples of the reference block and of the target block
    n_max = min(wlen, 2_000_000)                                   # processor.go:772 testChunkSize
    ref = [ctx.capture_download(s, 0, n_max) for s in range(3)]
    tgt = [ctx.capture_download(s, block, n_max) for s in range(3)]
    gomp = None
    try:
        gomp = ctypes.CDLL("libgomp.so.1")
    except OSError:
        pass

    def run(n, nthreads):
        if gomp is not None:
            gomp.omp_set_num_threads(int(nthreads))
        sig = [[o.iq_u8_to_c64(x[:2 * n]) for x in blk] for blk in (ref, tgt)]
        t0 = time.perf_counter()
        for blk in sig:
            for (i, j) in [(0, 1), (0, 2), (1, 2)]:
                o.cross_correlate(blk[i], blk[j])
        return time.perf_counter() - t0

    def calibrated(nthreads, budget):
        n = 20000
        t = run(n, nthreads)
        n_big = int(min(n_max, max(n, n * budget / max(t, 1e-3))))
        if n_big > 2 * n:
            n, t = n_big, run(n_big, nthreads)
        return n, t

    n1, t1 = calibrated(1, budget_s)
    # all cores: one thread per physical core, on at least the single-thread sample (a 20 000-sample probe on 256 threads
    # measures nothing but the fork/join cost of the filter loops)
    nn = int(min(n_max, 4 * n1))
    tn = run(nn, phys) if gomp is not None else t1 * nn / n1
    # --- same algorithm as the GPU path, float64, on the CPU cores (one (pair, window) per worker process)
    try:
        import multiprocessing as mp
        # one worker process per physical core (CPU-fft-N: all host cores); a worker holds
        # ~0.3 GB of float64 arrays for a 2 000 000-sample pair
        workers = max(1, phys)
        n_f = min(wlen, 2_000_000)
        segs = [ctx.capture_download(s, 0, n_f).tobytes() for s in range(3)]
        units = ([(segs[i], segs[j], max_lag) for (i, j) in [(0, 1), (0, 2), (1, 2)]] * ((workers + 2) // 3))[:max(workers, 3)]
        pool = mp.get_context("spawn").Pool(min(workers, len(units)))
        try:
            pool.map(_mode_b_f64_unit, units[:min(workers, len(units))], chunksize=1)      # start-up outside the clock
            t0 = time.perf_counter()
            pool.map(_mode_b_f64_unit, units, chunksize=1)
            tf = time.perf_counter() - t0
        finally:                                             # every child is ended and reaped on every path
            pool.terminate()
            pool.join()
        fft = {"value": round(len(units) * n_f / tf / 1e6, 3), "unit": "pair-Msamples/s",
               "cores": min(workers, len(units)),
               "sample": "float64 atan2 discriminator + numpy FFT cross-correlation (oracle/float_pipeline.py), %d (pair, window) "
                         "units of %d samples on %d worker processes, %.2f s" % (len(units), n_f, min(workers, len(units)), tf)}
    except Exception as e:                                                           # never fail the bench on the extra leg
        fft = {"error": repr(e)}
    return {
        "value": round(6 * n1 / t1 / 1e6, 4), "unit": "Msamples/s", "cores": 1, "kind": "port",
        "cpu_model": model, "physical_cores": phys, "hardware_threads": threads,
        "compare_against": "value (ONE thread: the reference is a single-threaded program); all_cores and same_algorithm_f64_fft are context",
        "sample": "oracle restatement of processor.go crossCorrelate (power gate, moving-average filter chain, time-domain "
                  "correlation), the reference's 6-call pattern: 3 pairs x {reference block, target block}, first %d samples "
                  "of each, same bytes as the GPU run, ONE thread (the reference is single-threaded), %.1f s" % (n1, t1),
        "all_cores": {"value": round(6 * nn / tn / 1e6, 4), "unit": "Msamples/s", "cores": phys,
                      "sample": "the same 6 calls, OpenMP inside each call, one thread per physical core (%d of %d hardware "
                                "threads), first %d samples, %.1f s" % (phys, threads, nn, tn)},
        "same_algorithm_f64_fft": fft,
    }, parity


def propagation_delays(stations, fs):
    """whole-sample propagation delay of every station from TX (what --sim fmdelay applies to the carrier)"""
    import tdoa_amd
    tx = tdoa_amd.capi.latlon_to_ecef(*TX)
    out = []
    for st in stations:
        p = tdoa_amd.capi.latlon_to_ecef(*st)
        dist = math.sqrt(sum((a - b) ** 2 for a, b in zip(tx, p)))
        out.append(int(round(dist / 299792458.0 * fs)))
    return out


def synth_torch_captures(ctx, torch, sim, S, block, seed0, delays):
    """capture bytes generated by torch in HBM and attached without a copy (returns the buffers: they must outlive ctx).
    random : uniform random bytes (every table entry of K1 equally likely)
    fm     : independent frequency-modulated carriers at half scale per station (what a well-set RTL-SDR gain delivers)
    fmdelay: ONE frequency-modulated carrier per block (the transmitter at TX), every station receiving it `delays[s]`
             samples late plus its own noise -- captures whose pairs correlate at lag delays[j] - delays[i]"""
    piece = 1 << 24
    bufs = [torch.empty(2 * 3 * block, dtype=torch.uint8, device="cuda") for _ in range(S)]

    def fm_phase(gen, n, phase0=0.0):
        # phi = running sum of a smoothed noise message (modulation index 1)
        msg = torch.randn(n + 63, device="cuda", generator=gen)
        msg = torch.nn.functional.conv1d(msg.view(1, 1, -1), torch.full((1, 1, 64), 1.0 / 8.0, device="cuda")).view(-1)
        return torch.cumsum(msg.double(), 0) + phase0

    def to_bytes(phi, gen):
        ph = torch.remainder(phi, 2.0 * math.pi).float()
        noise = (torch.rand(2 * ph.numel(), device="cuda", generator=gen) * 2 - 1) * 0.02
        iq = torch.stack([0.5 * torch.cos(ph), 0.5 * torch.sin(ph)], dim=1).view(-1) + noise
        return torch.clamp(torch.trunc(iq * 127.5 + 127.5), 0, 255).to(torch.uint8)

    if sim == "fmdelay":
        dmax = max(delays)
        for b in range(3):
            gen = torch.Generator(device="cuda")
            gen.manual_seed(seed0 * 8 + b)
            phi = torch.empty(block + dmax, dtype=torch.float64, device="cuda")       # the transmitter's phase, dmax samples early
            phase0 = 0.0
            for lo in range(0, block + dmax, piece):
                m = min(piece, block + dmax - lo)
                phi[lo:lo + m] = fm_phase(gen, m, phase0)
                phase0 = float(phi[lo + m - 1])
            for s_ in range(S):
                gn = torch.Generator(device="cuda")
                gn.manual_seed(seed0 * 8 + 64 * (s_ + 1) + b)
                off = dmax - delays[s_]                                                # station sample n = transmitter sample n - delay
                for lo in range(0, block, piece):
                    m = min(piece, block - lo)
                    bufs[s_][2 * (b * block + lo):2 * (b * block + lo + m)] = to_bytes(phi[off + lo:off + lo + m], gn)
            del phi
    else:
        for s_ in range(S):
            gen = torch.Generator(device="cuda")
            gen.manual_seed(seed0 + s_)
            phase0 = 0.0
            for lo in range(0, 3 * block, piece):
                m = min(piece, 3 * block - lo)
                if sim == "random":
                    bufs[s_][2 * lo:2 * (lo + m)] = torch.randint(0, 256, (2 * m,), dtype=torch.uint8, device="cuda", generator=gen)
                else:
                    phi = fm_phase(gen, m, phase0)
                    phase0 = float(phi[-1])
                    bufs[s_][2 * lo:2 * (lo + m)] = to_bytes(phi, gen)
    for s_ in range(S):
        ctx.capture_attach_device(s_, bufs[s_].data_ptr(), 3 * block)
    return bufs


def sample_clocks(run_steps):
    """shader clock and socket power while `run_steps()` keeps the GPU busy (rocm-smi polled from a thread; the timed
    region of a cfg2 run lasts 30 ms -- too short to poll -- so the same step is replayed for ~1.5 s right after it)"""
    import re
    import statistics
    import subprocess
    import threading
    samples, stop = [], threading.Event()
    dev = os.environ.get("HIP_VISIBLE_DEVICES", os.environ.get("ROCR_VISIBLE_DEVICES", "")).split(",")[0]

    def poll():
        while not stop.is_set():
            try:
                txt = subprocess.run(["/opt/rocm/bin/rocm-smi", "--showpower", "--showclocks", "--csv"], capture_output=True,
                                     text=True, timeout=5).stdout
                for line in txt.splitlines():
                    m = re.match(r"card(\d+),\((\d+)Mhz\),\d+,\((\d+)Mhz\),\d+,\((\d+)Mhz\),\d+,\((\d+)Mhz\),\w+,([\d.]+)", line)
                    if m:
                        samples.append((int(m.group(1)), int(m.group(4)), float(m.group(6))))
            except Exception:
                return
            time.sleep(0.1)

    th = threading.Thread(target=poll, daemon=True)
    th.start()
    run_steps()
    stop.set()
    th.join(timeout=10)
    if not samples:
        return None
    # the card under load: the one with the highest power draw (one GPU per box here; HIP_VISIBLE_DEVICES names it otherwise)
    cards = sorted({c for c, _, _ in samples})
    card = int(dev) if dev.isdigit() and int(dev) in cards else max(cards, key=lambda c: max(p for cc, _, p in samples if cc == c))
    busy = [(sc, pw) for c, sc, pw in samples if c == card and pw > 0.6 * max(p for cc, _, p in samples if cc == card)]
    if not busy:
        return None
    return {"sclk_MHz": statistics.median(sc for sc, _ in busy), "socket_W": statistics.median(pw for _, pw in busy),
            "samples": len(busy), "source": "rocm-smi polled during ~1.5 s of the same step replayed right after the timed region"}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, peaks, fixes):
    """--dump-outputs: what the timed region's last step handed its caller, one float32 / float64 array per field as
    <out_dir>/<name>.npy -- the peak records (windows x pairs) and, on multi-rank jobs, the solve of every capture set.
    The inputs are seeded, so two builds run with the same arguments can be compared array by array.  Past 64 MB the peak
    records are cut to a fixed, seeded sample of windows (peak_window_index.npy names them).  Returns the names written."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {}
    if peaks is not None:
        rows = np.arange(peaks.shape[0])
        row_bytes = peaks[:1].size * 20                                       # lag (as f64), abs_corr (f32), corr (f64)
        if peaks.shape[0] * row_bytes > DUMP_LIMIT_BYTES:
            rows = np.sort(np.random.default_rng(SEED_BASE).choice(peaks.shape[0], DUMP_LIMIT_BYTES // (row_bytes + 8), replace=False))
            arrays["peak_window_index"] = rows.astype(np.float64)
        arrays["peak_lag"] = peaks["lag"][rows].astype(np.float64)
        arrays["peak_abs_corr"] = peaks["abs_corr"][rows].astype(np.float32)
        arrays["peak_corr"] = peaks["corr"][rows].astype(np.float64)
    if fixes:
        arrays["solve_status"] = np.array([float(f[0]) for f in fixes])
        arrays["solve_lat_lon"] = np.array([[float(f[1][0]), float(f[1][1])] for f in fixes])
        arrays["solve_median_target_lags"] = np.array([np.asarray(f[3], dtype=np.float64) for f in fixes])
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return sorted(arrays)


def run_job(args, env, cfg_name, scaling, sim, steps, warmup, contract, full):
    """one job (configuration + sharding mode) on the process group `env`: captures, warm-up, timed region.  `contract`: the
    contract line's job, whose timed region is the step graph with event-record nodes around the dominant kernel (picked
    from an untimed per-kernel table first) and whose outputs --dump-outputs writes; `full` (--full): also the roofline
    object, the graph-replay leg, clocks, the end-to-end leg and the CPU baseline.  Returns (result dict for rank 0 | None,
    parity flag)."""
    import numpy as np
    import torch
    import tdoa_amd
    from tdoa_amd import sharding

    world, rank, device, backend, dist, use_dist = env["world"], env["rank"], env["device"], env["backend"], env["dist"], env["use_dist"]
    cfg = dict(CONFIGS[cfg_name])
    fs, wlen, max_lag = cfg["fs"], cfg["wlen"], args.max_lag
    S = cfg["stations"]
    block = int(args.seconds * fs) // 3 if args.seconds else cfg["block"]
    stations = station_table(S)
    ctx = tdoa_amd.Context(device=device, window_len=wlen, max_lag=max_lag, sample_rate=fs, windows_per_batch=args.batch)
    seed0 = SEED_BASE + (16 * rank if scaling == "weak" else 0)        # strong: every rank holds the SAME capture set
    delays = propagation_delays(stations, fs)
    attached = None                                                    # torch buffers the library reads in place
    if sim != "config":
        attached = synth_torch_captures(ctx, torch, sim, S, block, seed0, delays)
    else:
        for s in range(S):
            if cfg["sim"] == "weak":
                ctx.synth_weak_capture(s, block, stations[s], TX, seed0 + s, tgt_power=20000.0)
            else:
                ctx.synth_capture(s, block, stations[s], TX, seed0 + s)
    wpb, n_windows = ctx.num_windows()
    n_pairs = ctx.num_pairs()
    wl = min(wlen, block)
    job_samples = S * n_windows * wl                                    # station-samples one capture set holds
    samples_per_step = job_samples * (world if scaling == "weak" else 1)

    peak_bytes = n_windows * n_pairs * 16
    dev_peaks = torch.zeros(peak_bytes, dtype=torch.uint8, device="cuda")
    gathered = torch.zeros(peak_bytes * world, dtype=torch.uint8, device="cuda") if use_dist else None
    state = {"peaks": None, "fix": None}
    tgt_rows = np.arange(wpb, 2 * wpb)                                    # windows of the target block
    pair_list = [(i, j) for i in range(S) for j in range(i + 1, S)]

    def solve(pk):
        """downstream of the path (processor.go:892-926): median target-block lag per pair -> range differences ->
        least-squares position (3 stations: the reference's solver; more: tdoa_solve_nstation weighted by |corr|)"""
        lag = np.median(pk["lag"][tgt_rows], axis=0)
        wgt = np.maximum(np.median(pk["abs_corr"][tgt_rows], axis=0).astype(np.float64), 1e-12)
        rd = lag / fs * 299792458.0
        ref = tdoa_amd.capi.solve_3station(stations, rd) if S == 3 else tdoa_amd.capi.solve_nstation(stations, rd, weights=wgt)
        # the reference freezes ECEF Z at the centroid (processor.go:1004): a plane that misses a ground transmitter by
        # hundreds of metres; the fix that is CHECKED holds the position on the ellipsoid instead (tdoa_solve_surface)
        fix = tdoa_amd.capi.solve_surface(stations, rd, weights=wgt, height_m=sum(s_[2] for s_ in stations) / S)
        return fix + (lag, ref)

    def step():
        if not use_dist:
            state["peaks"] = ctx.process(0, 1, out_dev_ptr=dev_peaks.data_ptr(), want_host=True)     # peaks on the host
            return
        if scaling == "strong":
            ctx.process(rank, world, out_dev_ptr=dev_peaks.data_ptr(), want_host=False)
        else:
            ctx.process(0, 1, out_dev_ptr=dev_peaks.data_ptr(), want_host=False)
        if backend == "nccl":
            dist.all_gather_into_tensor(gathered, dev_peaks)        # RCCL over xGMI: per-pair peak records
        else:
            parts = [torch.empty(peak_bytes, dtype=torch.uint8) for _ in range(world)]
            dist.all_gather(parts, dev_peaks.cpu())
            gathered.copy_(torch.cat(parts))
        if scaling == "strong" and rank == 0:
            # other ranks' units are zero bytes in every part: the byte-wise maximum IS the owner merge
            merged = gathered.view(world, -1).amax(dim=0).cpu().numpy()
            state["peaks"] = sharding.bytes_as_peaks(merged, n_windows, n_pairs)
            state["fix"] = solve(state["peaks"])
        elif scaling == "weak" and rank == 0:
            # rank r's part is capture set r (windows r n_windows ... of the job): decode all, solve every set
            parts = gathered.cpu().numpy().reshape(world, -1)
            fixes = [solve(sharding.bytes_as_peaks(parts[r], n_windows, n_pairs)) for r in range(world)]
            state["peaks"] = sharding.bytes_as_peaks(parts[0], n_windows, n_pairs)
            state["fix"] = fixes[0]
            state["fixes"] = fixes

    def fence():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(n_steps):
        fence()
        t0 = time.perf_counter()
        for _ in range(n_steps):
            step()
        fence()
        dt_ = time.perf_counter() - t0
        if use_dist:
            tt = torch.tensor([dt_], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt_ = float(tt.item())
        return dt_

    for _ in range(warmup):
        step()
    table, dominant, timed_mode, table_steps, dominant_by = None, None, 0, steps, None
    if contract:
        # (untimed) every kernel scope of a few steps with events: the name of the dominant kernel, which the timed region
        # instruments (plain runs too: it is part of what the timed steps are), and the per-kernel table of --full's fields.
        # Kernels launched one by one, an event at every kernel boundary.
        ctx.profile_enable(True)
        ctx.profile_select(None)
        ctx.profile_reset()
        for _ in range(table_steps):
            step()
        torch.cuda.synchronize()
        table = ctx.profile()
        dominant = max(table.items(), key=lambda kv: kv[1]["ms"])[0]
        # timed region of the contract: the library's default path -- the whole step replayed as ONE hipGraph -- with two
        # event-record nodes spliced into the captured graph around the DOMINANT kernel (the roofline's launch durations,
        # measured live on the library's stream inside the timed steps).  The same steps without any event are timed right
        # after (graph_replay).  With TDOA_NO_GRAPH=1 (no step graph) or a runtime whose event-record nodes do not fire: the
        # launch-by-launch path with events around the same kernel.
        timed_mode = 2
        graph_marks_ok = os.environ.get("TDOA_NO_GRAPH") != "1"
        dominant_by = "the untimed kernel-by-kernel table"
        if graph_marks_ok:
            # The table is measured launch by launch; the timed path is the replayed graph, where the same kernels run a few per cent
            # apart from that (cfg2's two largest are within 5 % of each other and the table's order flipped from box to box).
            # So the two largest scopes of the table are each timed INSIDE the replayed graph for a few untimed steps, and the
            # larger one there is the dominant kernel the timed region instruments.
            ranked = [k for k, _ in sorted(table.items(), key=lambda kv: -kv[1]["ms"]) if table[k]["launches"]][:2]
            in_graph = {}
            for cand in ranked:
                ctx.profile_select([cand])
                ctx.profile_enable(2)
                step()                                                    # captures and instruments the graph (untimed)
                ctx.profile_reset()
                for _ in range(max(3, min(steps, 10))):
                    step()
                rec_c = ctx.profile()[cand]
                if rec_c["launches"]:
                    in_graph[cand] = rec_c["ms"] / max(3, min(steps, 10))
            if in_graph:
                dominant = max(in_graph.items(), key=lambda kv: kv[1])[0]
                dominant_by = "event-record nodes inside the replayed graph (%s)" % ", ".join("%s %.4f ms" % kv for kv in in_graph.items())
            ctx.profile_select([dominant])
            ctx.profile_enable(2)
            step()                                                        # the graph instrumented around the dominant scope
            ctx.profile_reset()
            step()
            graph_marks_ok = bool(ctx.profile()[dominant]["launches"])
        else:
            ctx.profile_select([dominant])
        if not graph_marks_ok:
            print("bench: graph-mode profiling unavailable (no step graph, or no event-record node fired); timing the "
                  "launch-by-launch path", file=sys.stderr)
            timed_mode = 1
            ctx.profile_enable(1)
            step()
        ctx.profile_reset()
    dt = timed(steps)
    prof_timed = None
    if contract:
        ctx.profile_enable(False)
        ctx.profile_select(None)
        prof_timed = ctx.profile()
        if not prof_timed[dominant]["launches"]:
            raise BenchCheckFailed("profiling recorded nothing for %s" % dominant)
    timed_peaks = None if state["peaks"] is None else state["peaks"].copy()     # what the contract's timed region produced
    timed_fix = state["fix"]
    timed_fixes = state.get("fixes") or ([timed_fix] if timed_fix is not None else [])
    dumped = None
    if contract and rank == 0 and args.dump_outputs:
        dumped = dump_outputs(args.dump_outputs, timed_peaks, timed_fixes)
    graph_leg = None
    if full and not args.no_graph_leg:
        step()                                                            # captures the graph
        dtg_first = timed(steps)                                          # (next to a collective the first replays of a new graph are slow)
        dtg = timed(steps)
        graph_leg = {"ms_per_step": round(dtg / steps * 1e3, 4), "value": round(samples_per_step / (dtg / steps) / 1e6, 2),
                     "identical_to_timed_path": None if timed_peaks is None else bool(np.array_equal(timed_peaks, state["peaks"])),
                     "first_pass_ms_per_step": round(dtg_first / steps * 1e3, 4),
                     "note": "the same steps, the same graph without the two event-record nodes; timed twice, the second pass counts "
                             "(the first replays of a newly instantiated graph are slow when collectives run between them)"}
    clocks, sustained = None, None
    if full and not args.no_clocks:
        # the contract's timed region lasts tens of milliseconds on cfg2 (20 x 2.6 ms): too short for anybody's sampler to see
        # the GPU busy.  The same step is replayed for ~1.5 s right after it; its time is reported (`sustained`) next to the
        # clocks and the socket power rocm-smi showed meanwhile.
        n_sustain = max(steps, int(1.5 / max(dt / steps, 1e-6)))          # the same count on every rank (dt is the max over ranks)
        box = {}

        def sustain():
            box["dt"] = timed(n_sustain)
        if rank == 0:
            clocks = sample_clocks(sustain)
        else:
            sustain()
        sustained = {"steps": n_sustain, "ms_per_step": round(box["dt"] / n_sustain * 1e3, 4),
                     "value": round(samples_per_step / (box["dt"] / n_sustain) / 1e6, 2), "seconds": round(box["dt"], 3),
                     "note": "the timed region's step (the same step graph, no event-record nodes) replayed back to back right after it, "
                             "barrier + synchronize on both sides, max over ranks"}

    if world > 1 and scaling == "strong" and n_windows >= world:
        # every rank's part must be what the owner merge expects: its own windows, zeros elsewhere
        mine = np.frombuffer(dev_peaks.cpu().numpy().tobytes(), dtype=tdoa_amd.capi.PEAK_DTYPE).reshape(n_windows, n_pairs)
        for wid in range(n_windows):
            if wid % world != rank and (mine[wid]["lag"].any() or mine[wid]["corr"].any()):
                raise BenchCheckFailed("rank %d of %d wrote a window it does not own (%d): nonzero windows %r"
                                 % (rank, world, wid, [w for w in range(n_windows) if mine[w]["lag"].any() or mine[w]["corr"].any()]))
    if world > 1 and scaling == "weak":
        got = torch.frombuffer(bytearray(gathered.cpu().numpy().tobytes()), dtype=torch.uint8).view(world, -1)
        if not torch.equal(got[rank], dev_peaks.cpu()):
            raise BenchCheckFailed("all-gather of peak records is inconsistent on rank %d" % rank)

    out, parity = None, None
    if rank == 0:
        ms_per_step = dt / steps * 1e3
        value = samples_per_step / (dt / steps) / 1e6
        n_fft, n1, n2 = ctx.plan_info()
        if use_dist and scaling == "strong":
            par = ("one capture set, windows dealt wid %% %d to the ranks, %s all-gather of the peak records, owner merge + "
                   "least-squares solve on rank 0, all inside the timed region" % (world, "RCCL" if backend == "nccl" else backend))
        elif use_dist:
            par = ("one job of %d x %d windows, window-major: rank r holds and processes capture set r (%d windows), %s all-gather of "
                   "the peak records, rank 0 decodes all of them and solves every set, all inside the timed region"
                   % (world, n_windows, n_windows, "RCCL" if backend == "nccl" else backend))
        else:
            par = "single GPU"
        data_note = {"config": "", "fm": "; capture bytes: independent half-scale FM carriers (torch)",
                     "random": "; capture bytes: uniform random (torch)",
                     "fmdelay": "; capture bytes: one half-scale FM carrier from TX, every station's copy delayed by its propagation "
                                "time (torch) -- the pairs correlate at the geometry's lags"}[sim]
        if sim == "config" and cfg["sim"] == "weak":
            data_note = ("; weak_signal_simulator.go model with tgt_power = 20000 where its example call passes 1000 "
                         "(weak_signal_simulator.go:298): at 1000 the target tone is below one LSB and every window is constant bytes")
        out = {
            "metric": "IQ Msamples/s through demod+xcorr", "value": round(value, 2), "unit": "Msamples/s",
            "n_gpus": world, "steps": steps, "warmup": warmup, "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True, "scaling": scaling, "vs_baseline": None, "dtype": "f32",      # K1: integer phase codes of pi/2^23 per step, exact in f32; transforms in f32
            "data": "synthetic",
            "config": {"workload": "%s%s, %d pairs x %d windows of %d samples, FFT N=%d (%dx%d), max_lag %d; peaks on the host%s"
                                   % (cfg["label"], " per GPU" if (scaling == "weak" and world > 1) else "", n_pairs, n_windows, wl,
                                      n_fft, n1, n2, max_lag, data_note),
                       "name": cfg_name, "capture_bytes": sim, "stations": S, "pairs": n_pairs, "windows": n_windows, "window_len": wl,
                       "fft_n": n_fft, "sample_rate": fs, "parallelism": par},
            "source_sha16": source_hash(),
            "k1_path": "single look (every capture byte read once; csrc/k1_single_look.hpp)" if ctx.last_k1(0)[1]
                       else "statistics pre-pass + discriminator in the column pass (capture bytes read twice)",
            "clocks": clocks, "sustained": sustained, "path_switches": path_switches() or None,
        }
        if contract and full:
            out["dominant_chosen_by"] = dominant_by
            out.update(roofline_fields(args, env, cfg_name, scaling, sim, table, prof_timed, dominant, timed_mode, table_steps, steps,
                                       dt, samples_per_step, n_fft, n1, n2, n_windows, n_pairs, S, wl, max_lag, graph_leg))
        if dumped is not None:
            out["dumped_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
        if timed_fix is not None:
            fixes = timed_fixes
            frc, flle, fit, flag, fref = timed_fix
            sol = {"status": int(frc), "lat": round(float(flle[0]), 6), "lon": round(float(flle[1]), 6), "iterations": int(fit),
                   "solver": "tdoa_solve_surface: weighted Gauss-Newton over all pairs, position held on the ellipsoid at the "
                             "stations' mean elevation",
                   "reference_solver": {"status": int(fref[0]), "lat": round(float(fref[1][0]), 6), "lon": round(float(fref[1][1]), 6),
                                        "note": "processor.go:932-1020 (3 stations) / its N-station form: ECEF X,Y with Z frozen at the "
                                                "centroid, 0.5 damping, 10 iterations -- also run inside the timed region"},
                   "median_target_lags": [float(x) for x in flag]}
            if sim == "fmdelay":
                want = np.array([delays[j] - delays[i] for (i, j) in pair_list], dtype=np.float64)
                errs = []
                for (rc_, lle_, _, lag_, _) in fixes:
                    a = tdoa_amd.capi.latlon_to_ecef(float(lle_[0]), float(lle_[1]), TX[2])
                    b = tdoa_amd.capi.latlon_to_ecef(TX[0], TX[1], TX[2])
                    errs.append(math.sqrt(sum((x - y) ** 2 for x, y in zip(a, b))))
                    if int(rc_) != 0 or not np.array_equal(np.asarray(lag_, dtype=np.float64), want) or errs[-1] > 150.0:
                        raise BenchCheckFailed("bench: the solve inside the timed region did not find the transmitter: status %d, lags %r "
                                         "(geometry: %r), fix (%.6f, %.6f), %.1f m from TX" % (int(rc_), list(lag_), list(want),
                                                                                               float(lle_[0]), float(lle_[1]), errs[-1]))
                sol.update({"expected_lags": [float(x) for x in want], "lags_equal_geometry": True,
                            "horizontal_error_m": round(max(errs), 1), "capture_sets_solved": len(fixes),
                            "note": "merge + least-squares solve inside the timed region; every pair's median target-block lag equals "
                                    "delay_j - delay_i of the synthetic geometry and the fix lies within 150 m of TX (one sample = 150 m "
                                    "of range) -- checked for every capture set, the run fails otherwise"})
            else:
                sol["note"] = ("the merge + least-squares solve run inside the timed region; these captures restate simulator.go "
                               "(unmodulated tones + noise, carrier PHASE delays only), so the peaks are noise peaks and a non-zero "
                               "status (7 = singular Jacobian, processor.go:997-999) is the solver's honest answer to them")
            out["solve"] = sol
        if full and world == 1 and not use_dist and not args.no_h2d and 2 * S * 3 * block <= (4 << 30):
            out["end_to_end_h2d"] = end_to_end_h2d(ctx, tdoa_amd, np, S, block, wlen, max_lag, fs, args.batch, device, timed_peaks)
        if full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"], parity = cpu_baseline_leg(ctx, timed_peaks, block, wl, max_lag, args.cpu_budget)
            out["parity_window0"] = parity
    ctx.close()
    del attached, dev_peaks, gathered
    torch.cuda.empty_cache()
    return out, parity


def end_to_end_h2d(ctx, tdoa_amd, np, S, block, wlen, max_lag, fs, batch, device, timed_peaks):
    """SURVEY 8d's secondary figure: the same job from HOST bytes (pageable buffers, the boundary a cgo caller hands over:
    tdoa_process_u8) to peaks on the host -- staging through pinned buffers, H2D over PCIe, the same step.  Never `value`."""
    caps = [ctx.capture_download(s, 0, 3 * block) for s in range(S)]
    with tdoa_amd.Context(device=device, window_len=wlen, max_lag=max_lag, sample_rate=fs, windows_per_batch=batch) as c2:
        c2.process_u8([x[:2 * 3 * min(block, 2 * wlen)] for x in caps])           # warm-up: plans, tables, staging buffers
        c2.process_u8(caps)                                                      # ... and the device buffers at full size
        t0 = time.perf_counter()
        pk = c2.process_u8(caps)
        dt = time.perf_counter() - t0
    n = S * pk.shape[0] * min(wlen, block)
    return {"value": round(n / dt / 1e6, 1), "unit": "Msamples/s", "seconds": round(dt, 4),
            "GB_per_s_h2d": round(sum(x.size for x in caps) / dt / 1e9, 2),
            "identical_to_timed_path": None if timed_peaks is None else bool(np.array_equal(pk, timed_peaks)),
            "note": "tdoa_process_u8 on pageable host buffers (%d x %.0f MB): staged H2D + the same step; link-bound, never `value`"
                    % (S, caps[0].size / 1e6)}


def roofline_fields(args, env, cfg_name, scaling, sim, table, prof_timed, dominant, timed_mode, table_steps, steps, dt,
                    samples_per_step, n_fft, n1, n2, n_windows, n_pairs, S, wl, max_lag, graph_leg):
    world = env["world"]
    prof = {k: {"ms": v["ms"] * steps / table_steps, "launches": v["launches"] * steps // table_steps, "bytes": v["bytes"] * steps / table_steps}
            for k, v in table.items()}                                   # the untimed table, scaled to `steps` steps
    prof[dominant] = prof_timed[dominant]                               # the dominant kernel: measured inside the timed region
    name, rec = dominant, prof_timed[dominant]                          # the roofline's kernel: the one that was timed live
    nc = n_fft // 2
    # kernels behind every profiling scope of the library on this plan (names as rocprofv3 prints them, no template suffix)
    hot = {}
    once = os.environ.get("TDOA_NO_K1_ONCE") != "1"
    if n1 == 4096:          # the radix-16 register kernels (fft_radix16.hpp); the column pass depends on N2
        fused_k1 = n2 in (256, 512, 2048, 2560, 3072, 4096) and os.environ.get("TDOA_NO_FUSED_K1") != "1" and max_lag > 1024
        if fused_k1:
            col = ["k_fwd_col512_k1"] if n2 == 512 else ["k_fwd_col256_k1"] + (["k_fwd_col_finish"] if n2 > 256 else [])
        else:
            col = (["k_fwd_col16x_c16"] if n2 <= 128 else ["k_fwd_col256_c16"] if n2 == 256 else ["k_fwd_colx_c16"] if n2 <= 1024
                   else ["k_fwd_col256_c16", "k_fwd_col_finish"])
        hot = {"k_fm_demod": ["k_once_estimate", "k_once_edges", "k_once_final"] if (fused_k1 and once and max_lag > 4095) else ["k_fm_demod"],
               "k_fwd_col": col, "k_fwd_row": ["k_fwd_row4096"],
               "k_inv_row_pair": ["k_inv_row_pair4096"], "k_inv_col_peak": ["k_inv_col_pruned"]}
    reach = max_lag                     # lags -(max_lag - 1) .. max_lag - 1 plus the refinement neighbours
    decimated = (n1 == 4096 and n2 in (256, 512, 2048, 2560, 3072, 4096) and reach > 4095 and os.environ.get("TDOA_NO_DECIMATE") != "1"
                 and decimation_fits(n1 * n2, max_lag))
    if decimated:     # K3 + 16:1 FIR decimation of the pair spectrum, then an Nc/16-point inverse;
        #               on the 4096 x 4096 plan the FIR walks the columns of the spectrum (dec_stream.hpp)
        #               the FIR walks the columns of the spectrum (dec_stream.hpp) on the 4096 x 4096 plan and wherever a window
        #               carries more pairs than stations (tdoa_mi355x.hip dec_walks_columns); else 4096-bin tiles in LDS
        #               ... and, with the stations' rows staged in LDS, from three stations on (every bench job is a uniform batch)
        can_stage = os.environ.get("TDOA_NO_DEC_STAGED") != "1" and 3 <= S <= 16
        cols = os.environ.get("TDOA_NO_DEC_COLS") != "1" and (n2 in (2048, 2560, 3072, 4096) or n_pairs > S or can_stage
                                                              or os.environ.get("TDOA_DEC_COLS_ALWAYS") == "1")
        staged = cols and os.environ.get("TDOA_NO_DEC_STAGED") != "1" and S <= 16
        hot = dict(hot, k_fwd_row=["k_fwd_row4096_unpack"],
                   k_inv_row_pair=["k_pair_decimate_staged" if staged else "k_pair_decimate_cols" if cols else "k_pair_decimate16"],
                   k_inv_col_peak=["k_inv_rows_plain_r8", "k_small_col_peak", "k_small_rows_col_peak"])
    if max_lag <= 1024 and n1 == 4096:
        # segment form; with 3+ pairs per window the station transforms are shared (quads)
        hot = dict(hot, k_inv_row_pair=["k_xcorr_segments_quad" if n_pairs >= 3 and os.environ.get("TDOA_NO_SEGMENT_QUADS") != "1"
                                        else "k_xcorr_segments"], k_inv_col_peak=["k_segments_reduce"])
    roof, pmc_total = None, None
    if rec["launches"]:
        requested = rec["bytes"] / rec["launches"]                      # the library's per-kernel byte model: what the launch ASKS for
        avg_s = rec["ms"] / rec["launches"] / 1e3
        kernels = hot.get(name, [name])
        # a step may take several launch groups of windows (cfg3: 4, cfg5: 8): everything here is per LAUNCH
        windows_per_launch = n_windows * steps / rec["launches"]
        # HBM side of a pair step whose P pairs share S station spectra: each spectrum comes from memory once (its other
        # readers are served by L2 / Infinity Cache), the pair's own output is written -- the compulsory bytes of the launch
        compulsory = requested
        if name == "k_inv_row_pair" and n_pairs > 0:
            out_per_pair = 8.0 * nc
            if decimated:       # G (Nc/16 points) + the neighbour shares: X[12][4096] behind the column walk, E[N2][12] behind the tiles
                out_per_pair = 8.0 * nc / 16 + 8.0 * 12 * (4096 if hot["k_inv_row_pair"][0] in ("k_pair_decimate_cols", "k_pair_decimate_staged") else n2)
            compulsory = min(requested, windows_per_launch * (S * 8.0 * nc + n_pairs * out_per_pair))
        standard = (args.seconds is None and args.batch == 0 and world == 1 and max_lag == 20000 and sim == "config"
                    and not path_switches())
        traffic, src, sq = None, None, None
        if standard and name in hot:
            traffic, src, pmc_total = pmc_traffic(cfg_name, kernels)
            sq = sq_issue(cfg_name, kernels[0])
        # `achieved` / `frac` (the contract): ALGORITHMIC = compulsory bytes of the launch -- every operand from memory once,
        # every result written once -- over the HIP-event time of the launch.  `traffic` = what the memory-side counters saw for
        # the same launch; `traffic_over_algorithmic` above 1.25 names wasted re-reads (cfg4 / cfg5's pair step), `hbm_frac` is
        # the rate the HBM side actually ran at.  Neither can exceed 1 (rounds 2-3 printed request rates: 1.05 / 1.17).
        achieved = compulsory / avg_s / 1e9
        hbm_side = (traffic if traffic is not None else compulsory) / avg_s / 1e9
        limiter = None
        if sq is not None:
            limiter = "valu_issue" if sq["valu_issue_frac"] > max(0.6, hbm_side / HBM_FILL_GBS) else "hbm"
        roof = {"bound": "hbm", "kernel": " + ".join(kernels),
                "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                "bytes_source": ("compulsory bytes of the launch: every station spectrum from memory once + the pairs' outputs (its %d "
                                 "pairs per window re-read the spectra; whether on-die or not is what `traffic` shows)" % n_pairs
                                 if compulsory < requested else
                                 "the library's byte model of the launch (every operand streamed once, every result written once)"),
                "frac_of_measured_achievable": round(achieved / 6290.0, 4),   # guide: 6.29 TB/s achievable
                "frac_of_fill_rate": round(achieved / HBM_FILL_GBS, 4),
                "traffic": traffic, "traffic_source": None if traffic is None else "PMC (FETCH_SIZE + WRITE_SIZE, %s)" % src,
                "traffic_note": src if traffic is None else None,
                "traffic_over_algorithmic": None if traffic is None else round(traffic / compulsory, 3),
                "hbm_GBps": round(hbm_side, 1), "hbm_frac": round(hbm_side / HBM_PEAK_GBS, 4),
                "requested_GBps": round(requested / avg_s / 1e9, 1),          # request rate: operands asked for, wherever they come from
                "valu_issue_frac": None if sq is None else sq["valu_issue_frac"],
                "valu_instructions_per_wave": None if sq is None else sq["valu_instructions_per_wave"],
                "lds_conflict_frac": None if sq is None else sq["lds_conflict_frac"],
                "sq_source": None if sq is None else sq["source"],
                "limiter": limiter,
                "algorithmic_bytes_per_launch": compulsory, "requested_bytes_per_launch": requested,
                "avg_launch_us": round(avg_s * 1e6, 2), "launches": rec["launches"],
                "kernels_ms_per_step": {k: round(v["ms"] / steps, 4) for k, v in prof.items()},
                "kernels_ms_per_step_source": "%s: HIP events inside the timed region; the others: %d untimed steps launched kernel by "
                                              "kernel with an event at every boundary" % (name, table_steps),
                "note": "achieved / frac = algorithmic (compulsory) bytes of the launch / HIP-event time / 8 TB/s.  traffic = memory-side "
                        "counters of the same launch (profiles/, same kernel sources); hbm_GBps = traffic / the same time.  "
                        "requested_GBps = the operands the launch asks for / the same time (a request rate: on-die hits included).  "
                        "valu_issue_frac = share of the kernel's time its SIMDs spend issuing vector instructions (SQ counters "
                        "in profiles/, same kernel sources): limiter = valu_issue when that share exceeds both 0.6 and the HBM side's "
                        "share of the 5.8 TB/s a plain fill sustains"}
    # every scope of the step next to the dominant one: HBM-side rate and issue share from the same counter files, times from
    # the untimed kernel-by-kernel table (the dominant scope: from inside the timed region).  cfg2's two largest kernels are
    # within 3 % of each other -- one at the HBM roof, one bound by instruction issue -- and which of them is "dominant"
    # changes from box to box; this table shows both.
    by_kernel = None
    standard = (args.seconds is None and args.batch == 0 and world == 1 and max_lag == 20000 and sim == "config"
                and not path_switches())
    if standard and hot:
        by_kernel = []
        for scope, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"]):
            if not v["launches"] or scope not in hot:
                continue
            tr, _, _ = pmc_traffic(cfg_name, hot[scope])
            sqk = sq_issue(cfg_name, hot[scope][0])
            t_s = v["ms"] / v["launches"] / 1e3
            gbps = None if tr is None else tr / t_s / 1e9
            by_kernel.append({"scope": scope, "kernel": " + ".join(hot[scope]), "ms_per_step": round(v["ms"] / steps, 4),
                              "timed": "inside the timed region" if scope == dominant else "untimed table",
                              "hbm_GBps": None if gbps is None else round(gbps, 1),
                              "frac": None if gbps is None else round(gbps / HBM_PEAK_GBS, 4),
                              "valu_issue_frac": None if sqk is None else sqk["valu_issue_frac"],
                              "limiter": None if (sqk is None or gbps is None) else
                                         ("valu_issue" if sqk["valu_issue_frac"] > max(0.6, gbps / HBM_FILL_GBS) else "hbm")})
    # whole-pipeline algorithmic bytes: k = ceil(log2 N / 12) passes of 4096-point tiles, e = 4 B:
    # 2L + e N (2k - 1) per station-window, e N 2k per pair-window  (k = 2: 2L + 12N and 16N; k = 3: 2L + 20N and 24N)
    k_pass = max(2, math.ceil(math.log2(n_fft) / 12.0))
    units_w = n_windows * (world if scaling == "weak" else 1)
    a_bytes = units_w * (S * (2 * wl + 4 * n_fft * (2 * k_pass - 1)) + n_pairs * 4 * n_fft * 2 * k_pass)
    return {
        "timed_path": ("the whole step replayed as one hipGraph (the library's default path) with event-record nodes around the "
                       "dominant kernel (the roofline's source)" if timed_mode == 2 else
                       "kernels launched one by one, HIP events around the dominant kernel's launches (the roofline's source)")
                      + "; the other kernels' times come from %d untimed steps launched kernel by kernel with an event at every "
                        "boundary; graph_replay: the whole step replayed as one hipGraph without any event" % table_steps,
        "graph_replay": graph_leg,
        # SURVEY.md 8d byte model (a fixed price list per sample, NOT what this pipeline moves: the decimated inverse and
        # the fused K1 move less) -- kept under its own name
        "pipeline_survey_model_GBps": round(a_bytes / (dt / steps) / 1e9, 1),
        # the bytes the launched kernels are charged with by the library (per-kernel figures of tdoa_profile_get: the
        # decimated pair step at its own 16.5 Nc per pair-window, the fused K1 with no code round trip): a request rate
        "pipeline_kernel_bytes_GBps": round(sum(v["bytes"] for v in prof.values()) / max(steps, 1) / (dt / steps) / 1e9, 1),
        # HBM side of the whole step: memory-side counters of every kernel of a step (profiles/, same sources) / step time
        "pipeline_pmc_GBps": None if not pmc_total else round(pmc_total / (dt / steps) / 1e9, 1),
        "pipeline_frac_of_hbm_peak": None if not pmc_total else round(pmc_total / (dt / steps) / 1e9 / HBM_PEAK_GBS / world, 4),
        # SURVEY.md 8d secondary figure: pair-samples correlated per second (P*W*L/t), whole job
        "pair_Msamples_per_s": round(samples_per_step / S * n_pairs / (dt / steps) / 1e6, 2),
        "roofline": roof,
        "roofline_by_kernel": by_kernel,
    }


def same_config_one_gpu(cfg_name):
    """the one-GPU rate of a configuration from the newest committed bench line of this round's collection -- only if it was
    taken on the current kernel sources"""
    f = _latest_profile("*_%s_bench.json" % cfg_name)
    if not f:
        return {"value": None, "note": "no committed one-GPU line for %s" % cfg_name}
    try:
        ref = json.loads(open(f).read().strip().splitlines()[-1])
        if ref.get("n_gpus") != 1 or ref.get("config", {}).get("name") != cfg_name:
            return {"value": None, "note": "%s is not a one-GPU %s line" % (os.path.basename(f), cfg_name)}
        if ref.get("source_sha16") != source_hash():
            return {"value": None, "source": "profiles/" + os.path.basename(f),
                    "note": "stale: taken on other kernel sources (%.1f Msamples/s there)" % ref["value"]}
        return {"value": ref["value"], "ms_per_step": ref["ms_per_step"], "source": "profiles/" + os.path.basename(f),
                "note": "one MI355X, `bench.py --gpus 1 --config %s`, same kernel sources" % cfg_name}
    except (OSError, ValueError, KeyError, IndexError):
        return {"value": None, "note": "unreadable: %s" % os.path.basename(f)}


def launch_ranks(gpus, argv, environ=None, run=None):
    """`bench.py --gpus N` by itself: N > 1 with no WORLD_SIZE in the environment means the caller did not start the ranks, so
    this process starts `python -m torch.distributed.run --nproc-per-node N bench.py <same arguments>` as a CHILD (never an
    exec, and before torch or any HIP call has been touched: a process that has initialised the GPU must not be replaced),
    passes its output through and returns its exit code.  Under a launcher (WORLD_SIZE set) the two must agree.
    Returns None when this process is a rank and should go on."""
    environ = os.environ if environ is None else environ
    ws = environ.get("WORLD_SIZE")
    if ws is not None:
        if int(ws) != gpus:
            print("bench.py: --gpus %d but WORLD_SIZE=%s: start one rank per GPU (torch.distributed.run --nproc-per-node %d) or "
                  "drop WORLD_SIZE and let bench.py start them" % (gpus, ws, gpus), file=sys.stderr)
            return 2
        return None
    if gpus <= 1:
        return None
    import socket
    import subprocess
    port = environ.get("MASTER_PORT")
    if not port:
        with socket.socket() as sk:                      # a free port on the loopback interface
            sk.bind(("127.0.0.1", 0))
            port = str(sk.getsockname()[1])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
           "--master-addr", "127.0.0.1", "--master-port", port, os.path.abspath(__file__)] + list(argv)
    print("bench.py: starting %d ranks: %s" % (gpus, " ".join(cmd)), file=sys.stderr)
    return (run or subprocess.call)(cmd, env=dict(environ))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default: the config's); ms_per_step = their time / steps")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", choices=sorted(CONFIGS), default=None)
    ap.add_argument("--scaling", choices=("strong", "weak"), default=None)
    ap.add_argument("--seconds", type=float, default=None, help="capture length per station (overrides the config)")
    ap.add_argument("--batch", type=int, default=0, help="windows per launch group (0 = library default)")
    ap.add_argument("--max-lag", type=int, default=20000, help="search range in samples (reference: 20000, processor.go:633)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline figure does not need: roofline and per-kernel fields, the "
                         "graph-replay leg, clocks, the end-to-end leg from host buffers, the CPU baseline with the window-0 "
                         "parity check and, at N > 1, the sharded cfg4 job")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and its parity check")
    ap.add_argument("--no-graph-leg", action="store_true", help="with --full: skip the graph replay without event-record nodes")
    ap.add_argument("--no-clocks", action="store_true", help="with --full: skip the ~1.5 s sustained replay that samples clock and power")
    ap.add_argument("--no-h2d", action="store_true",
                    help="with --full: skip the end-to-end leg from host buffers (SURVEY 8d secondary figure)")
    ap.add_argument("--no-sharded-leg", action="store_true", help="with --full at N > 1: only the contract line's job, no sharded cfg4 job")
    ap.add_argument("--cpu-budget", type=float, default=10.0)
    ap.add_argument("--sim", choices=("config", "fm", "random", "fmdelay"), default=None,
                    help="capture bytes: 'config' = the config's simulator (+-1..3 LSB tones + noise; the default on one GPU), 'fm' = "
                         "independent frequency-modulated carriers at half scale (what a well-set RTL-SDR gain delivers), 'random' = "
                         "uniform random bytes (every table entry of K1 equally likely), 'fmdelay' = one FM carrier from TX delayed "
                         "per station by its propagation time (the default of multi-rank jobs: the solve has a position to find)")
    ap.add_argument("--force-dist", action="store_true",
                    help="at --gpus 1: initialise torch.distributed (nccl = RCCL, world size 1) and run the multi-GPU step -- "
                         "tdoa_process(rank, world), all_gather_into_tensor of the peak records, owner merge, solve -- on one GPU")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (peak records; the solve on multi-rank jobs) as "
                         "DIR/<name>.npy in float32 / float64, at most 64 MB, for comparing two builds output by output")
    args = ap.parse_args(argv)
    if args.steps is not None and args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")
    return args


def main():
    args = parse_args()

    rc = launch_ranks(args.gpus, sys.argv[1:])
    if rc is not None:
        sys.exit(rc)

    import torch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    # The default at every N is BASELINE config 2, WEAK-scaled: one job of N x 99 windows, window-major -- rank r holds and
    # processes its own 99 windows (its own capture set, different seeds), the peak records are all-gathered over RCCL and
    # rank 0 decodes all of them and solves every set.  Per-GPU work is fixed, so value(N) / (N value(1)) is the scaling
    # efficiency.  `--config cfg4 --scaling strong` is BASELINE config 4 as written: ONE 8-station capture set, its windows
    # dealt wid % N to the ranks; the default multi-rank run times it too (sharded_cfg4).
    # stdout carries ONE line, the JSON: RCCL writes its version banner and its warnings ("Missing iommu=pt ...") to fd 1, gloo
    # its rank chatter -- everything that is not the result goes to stderr from here on, at the descriptor level
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    cfg_name = args.config or "cfg2"
    scaling = args.scaling or "weak"
    steps = args.steps if args.steps is not None else CONFIGS[cfg_name]["steps"]
    # one rank per GPU; TDOA_BENCH_BACKEND=gloo is a rehearsal mode (several ranks may then share
    # a GPU and the peak records travel through host memory) -- the driver always runs nccl (= RCCL)
    backend = os.environ.get("TDOA_BENCH_BACKEND", "nccl")
    device = local_rank % torch.cuda.device_count() if backend == "gloo" else local_rank
    torch.cuda.set_device(device)
    dist = None
    use_dist = world > 1 or args.force_dist
    if use_dist:
        import torch.distributed as dist
        if os.environ.get("NCCL_DEBUG", "VERSION").upper() == "VERSION":      # RCCL's version banner goes to STDOUT: keep it off the JSON line
            os.environ["NCCL_DEBUG"] = "WARN"
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        kw = {} if world > 1 else {"rank": 0, "world_size": 1}
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", device), **kw)
        else:
            dist.init_process_group(backend=backend, **kw)
    env = {"world": world, "rank": rank, "device": device, "backend": backend, "dist": dist, "use_dist": use_dist}
    sim = args.sim or ("fmdelay" if use_dist else "config")

    def agreed(job):
        """run a job; a failed check on ANY rank ends every rank with a non-zero status (the others would otherwise sit in the
        next collective until the launcher kills them)"""
        err, res = None, (None, None)
        try:
            res = job()
        except BenchCheckFailed as e:
            err = "rank %d: %s" % (rank, e)
            print("bench: " + err, file=sys.stderr)
        if use_dist:
            ok = torch.tensor([0 if err else 1], dtype=torch.int32, device="cuda" if backend == "nccl" else "cpu")
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if int(ok.item()) == 0:
                dist.destroy_process_group()
                raise SystemExit(err or "rank %d: a check failed on another rank" % rank)
        elif err:
            raise SystemExit(err)
        return res

    out, parity = agreed(lambda: run_job(args, env, cfg_name, scaling, sim, steps, args.warmup, contract=True, full=args.full))
    # the sharded job BASELINE config 4 names, in the same run (default multi-rank invocation with --full only)
    if args.full and use_dist and args.config is None and args.scaling is None and not args.no_sharded_leg:
        s_steps = min(steps, CONFIGS["cfg4"]["steps"])
        sh, _ = agreed(lambda: run_job(args, env, "cfg4", "strong", sim, s_steps, 1, contract=False, full=False))
        if rank == 0:
            one = same_config_one_gpu("cfg4")
            out["sharded_cfg4"] = {
                "value": sh["value"], "unit": "Msamples/s", "ms_per_step": sh["ms_per_step"], "steps": s_steps, "scaling": "strong",
                "config": sh["config"], "solve": sh.get("solve"),
                "same_config_one_gpu": one,
                "efficiency_vs_same_config_one_gpu": None if not one.get("value") else round(sh["value"] / (world * one["value"]), 4),
                "note": "BASELINE config 4 as written, timed right after the contract line's job in the same process group: ONE "
                        "8-station capture set, windows dealt wid % N, one all-gather of the peak records, owner merge and "
                        "N-station solve on rank 0, all inside the timed region"}
    if rank == 0 and os.environ.get("TDOA_STG_PROF"):
        # measurement build of the staged column walk (-DTDOA_STG_TIMING, TDOA_LIB_VARIANT): its wave-cycle counters, to stderr
        import ctypes
        import tdoa_amd
        lib = tdoa_amd.capi.load()
        if hasattr(lib, "tdoa_debug_stg_prof"):
            buf = (ctypes.c_ulonglong * 8)()
            lib.tdoa_debug_stg_prof(buf)
            print("stg_prof " + " ".join(str(v) for v in buf), file=sys.stderr)
        else:
            print("TDOA_STG_PROF: the loaded library is not a -DTDOA_STG_TIMING build (TDOA_LIB_VARIANT)", file=sys.stderr)
    if rank == 0:
        if args.full and world > 1:
            out["same_config_one_gpu"] = same_config_one_gpu(cfg_name)
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if parity is False:
        raise SystemExit("parity check of window 0 against the oracle FAILED")


if __name__ == "__main__":
    main()
