#!/usr/bin/env python3
"""ms per tdoa_group_process against Context.process in the same run, on BASELINE config 2's geometry (3 stations x 100 s at
2 Msps, 99 windows of 2 000 000 samples, +-20 000 lags), captures synthesised on every member through tdoa_group_member.
Legs: a group of one member on device 0 next to two single contexts, one made before the group and one after (the three
alternated round by round, so they see the same box), groups of 2..M members that all share device 0, and -- when more
than one device is visible -- groups over devices 0..k-1.  Each group's peaks are compared byte for byte with the single
context's.  One JSON line per leg; times are medians over R rounds of N calls, host copy of the peaks included.
usage: scripts/time_group.py [--steps N] [--rounds R] [--shared M]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tdoa-geolocation_amd"))
import numpy as np  # noqa: E402
import tdoa_amd  # noqa: E402

ST = [(41.18660274289527, -95.96064116595667, 355.69), (41.24669616513154, -96.08366304481238, 329.0),
      (41.32916620016985, -96.03513381562004, 373.18)]
TX = (41.20, -96.00, 400.0)
BLOCK = 66_666_666
PARAMS = dict(sample_rate=2e6, window_len=2_000_000, max_lag=20000)


def synth(ctx):
    for s in range(3):
        ctx.synth_capture(s, BLOCK, ST[s], TX, 0x5D0A0000 + s)


def timed(fn, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()                                 # returns after the peaks are on the host (a stream synchronise)
    return (time.perf_counter() - t0) / steps * 1e3


def group(devices):
    g = tdoa_amd.Group(devices, **PARAMS)
    for k in range(len(devices)):
        synth(g.member(k))
    return g


def leg(name, devices, fn, want, steps, rounds, ref_ms):
    got = fn()                               # warm-up: captures the step graphs
    fn()
    ms = [timed(fn, steps) for _ in range(rounds)]
    out = {"leg": name, "devices": devices, "ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3),
           "ms_max": round(max(ms), 3), "over_context": round(statistics.median(ms) / ref_ms, 4),
           "identical": got.tobytes() == want.tobytes()}
    print(json.dumps(out), flush=True)
    return out


def main():
    args = sys.argv[1:]
    opt = {"--steps": 40, "--rounds": 7, "--shared": 4}
    for k in opt:
        if k in args:
            i = args.index(k)
            opt[k] = int(args[i + 1])
            del args[i:i + 2]
    steps, rounds = opt["--steps"], opt["--rounds"]
    n_dev = tdoa_amd.capi.load().tdoa_device_count()
    print(json.dumps({"device_count": n_dev, "steps": steps, "rounds": rounds}), flush=True)

    # a group of one against single contexts, through the C calls a host makes (one preallocated output), alternated
    # round by round; the second context is made after the group's member, so that a difference that comes from where a
    # context's buffers landed shows as a difference between the two contexts
    L = tdoa_amd.capi.load()
    c = tdoa_amd.Context(**PARAMS)
    synth(c)
    want = c.process()
    out = np.zeros_like(want)
    ptr = out.ctypes.data_as(C.c_void_p)
    g1 = group([0])
    c2 = tdoa_amd.Context(**PARAMS)
    synth(c2)
    calls = {"context": lambda: c._chk(L.tdoa_process(c._h, 0, 1, ptr, None)),
             "group1": lambda: g1._chk(L.tdoa_group_process(g1._h, ptr)),
             "context_made_later": lambda: c2._chk(L.tdoa_process(c2._h, 0, 1, ptr, None))}
    ms = {k: [] for k in calls}
    for fn in calls.values():
        fn()
        fn()
    for _ in range(rounds):
        for k, fn in calls.items():
            ms[k].append(timed(fn, steps))
    ident = g1.process().tobytes() == want.tobytes() and c2.process().tobytes() == want.tobytes()
    g1.close()
    c2.close()
    c.close()
    ref = statistics.median(ms["context"])
    line = {"leg": "context_vs_group_of_one", "identical": ident}
    for k, v in ms.items():
        line[k + "_ms_median"] = round(statistics.median(v), 3)
        line[k + "_ms"] = [round(x, 3) for x in v]
    line["group1_over_context"] = round(statistics.median(ms["group1"]) / ref, 4)
    line["group1_over_context_made_later"] = round(statistics.median(ms["group1"]) / statistics.median(ms["context_made_later"]), 4)
    print(json.dumps(line), flush=True)

    for m in range(2, opt["--shared"] + 1):  # members sharing device 0
        g = group([0] * m)
        leg("shared_device0_x%d" % m, [0] * m, g.process, want, steps, rounds, ref)
        g.close()
    for k in range(2, n_dev + 1):            # one member per device
        g = group(list(range(k)))
        leg("devices_0_to_%d" % (k - 1), list(range(k)), g.process, want, steps, rounds, ref)
        g.close()


if __name__ == "__main__":
    main()
