#!/usr/bin/env python3
"""ms per step of tdoa_process, tdoa_process_peaks(k = 8, min_separation = 8) and tdoa_process_lags on the window geometry
of BASELINE configs 2 and 4 (synthetic captures on the device, one GPU).  The graphs replay; host copies are included,
as a caller sees them.   usage: scripts/time_peaks.py [cfg2] [cfg4] [--steps N]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tdoa-geolocation_amd"))
try:
    import torch          # before the library: the process keeps torch's HIP runtime (bench.py does the same)
except Exception:         # pragma: no cover - the device-output leg is skipped
    torch = None
import numpy as np
import tdoa_amd

ST = [(41.18660274289527, -95.96064116595667, 355.69), (41.24669616513154, -96.08366304481238, 329.0),
      (41.32916620016985, -96.03513381562004, 373.18)]
TX = (41.20, -96.00, 400.0)
CONFIGS = {"cfg2": 3, "cfg4": 8}        # stations; 2 Msps, 3 blocks of 66 666 666 samples, 2 000 000-sample windows


def timed(fn, steps):
    fn()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    return (time.perf_counter() - t0) / steps * 1e3


def run(name, steps):
    n_st = CONFIGS[name]
    c = tdoa_amd.Context(sample_rate=2e6, window_len=2_000_000, max_lag=20000)
    rng = np.random.default_rng(1)
    for s in range(n_st):
        lle = ST[s] if s < 3 else (41.25 + 0.1 * rng.standard_normal(), -96.0 + 0.1 * rng.standard_normal(), 350.0)
        c.synth_capture(s, 66_666_666, lle, TX, 0x5D0A0000 + s)
    wpb, W = c.num_windows()
    P = c.num_pairs()
    lags = np.zeros((W, P, 2 * 20000 - 1), dtype=np.float32)
    lags_host = lags.ctypes.data_as(tdoa_amd.capi.C.POINTER(tdoa_amd.capi.C.c_float))
    out = {"config": name, "stations": n_st, "pairs": P, "windows": W,
           "surface_MB": round(W * P * (2 * 20000 - 1) * 4 / 1e6, 1)}
    out["process_ms"] = round(timed(lambda: c.process(), steps), 3)
    out["process_peaks_ms"] = round(timed(lambda: c.process_peaks(8, 8), steps), 3)
    out["process_lags_ms"] = round(timed(lambda: c._chk(c._L.tdoa_process_lags(c._h, 0, 1, lags_host, None)), steps), 3)
    out["process_lags_device_ms"] = None
    if torch is not None:
        dev = torch.empty(W * P * (2 * 20000 - 1), dtype=torch.float32, device="cuda")
        out["process_lags_device_ms"] = round(timed(lambda: c._chk(c._L.tdoa_process_lags(c._h, 0, 1, None, dev.data_ptr())), steps), 3)
    print(json.dumps(out), flush=True)
    c.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    steps = 10
    if "--steps" in args:
        i = args.index("--steps")
        steps = int(args[i + 1])
        del args[i:i + 2]
    for name in args or ["cfg2", "cfg4"]:
        run(name, steps)
