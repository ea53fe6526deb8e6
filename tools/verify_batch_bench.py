#!/usr/bin/env python3
"""Proofs per second of p2gpu_verify_batch on the GPU beside a loop of p2gpu_verify on 1 and on 16 host threads, same proofs,
same machine.  Prints one JSON line.

    python tools/verify_batch_bench.py [--circuits 13:arith,17:sha] [--batches 1,64,1024] [--window 0.5] [--step-timeout 300]

Each circuit is measured in a child process of its own under `timeout`: it proves the synthetic circuit on the GPU -- eight
witnesses that differ in a free wire cell (the synthetic circuits take no public inputs or seeds), repeated up to the batch
size --, verifies every batch size on the device, once more with the handle's "profile" knob (2: every launch) for the times of
the two kernels, and then runs the host loops.  A figure is never one call: after the warm-up calls the same call is repeated
back to back until --window seconds have passed (five calls at least), and the median, the fastest and the slowest call are
reported; proofs per second are taken from the median."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P = 0xFFFFFFFF00000001


def windowed(call, window, warm=2):
    """call() -> seconds, repeated back to back for `window` seconds: {median, min, max} in ms and the number of calls"""
    for _ in range(warm):
        call()
    ts, t_end = [], time.perf_counter() + window
    while len(ts) < 5 or time.perf_counter() < t_end:
        ts.append(call())
    ts.sort()
    return {"ms": round(ts[len(ts) // 2] * 1e3, 3), "ms_min": round(ts[0] * 1e3, 3), "ms_max": round(ts[-1] * 1e3, 3), "calls": len(ts)}


def host_loop(lib, handle, proofs, threads):
    """seconds for one p2gpu_verify per proof, the proofs dealt round-robin to `threads` threads"""
    import numpy as np

    bufs = [np.frombuffer(p, dtype=np.uint8) for p in proofs]
    bad = []

    def work(k):
        for b in bufs[k::threads]:
            if lib.p2gpu_verify(handle, b.ctypes.data, b.size):
                bad.append(k)

    ts = [threading.Thread(target=work, args=(k,)) for k in range(threads)]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    dt = time.perf_counter() - t0
    assert not bad, "the host verifier rejected a proof"
    return dt


def measure(d, mix, batches, window):
    import numpy as np

    import __graft_entry__ as entry

    pkg = entry.load_package()
    lib = pkg.load_library()
    blob, wires = pkg.make_circuit(d, mix, 7)[:2]
    cd = pkg.CircuitData(blob)
    vd = cd.verifier_data()
    distinct = []
    for k in range(8):
        w = wires.copy()
        w[-1, 3 + k] = (int(w[-1, 3 + k]) + k) % P
        try:
            distinct.append(cd.prove(w).to_bytes())
        except pkg.P2GpuError:  # the cell is not free in this mix: the unchanged witness again
            distinct.append(cd.prove(wires).to_bytes())
    out = {"circuit": "synth(%d, %s)" % (d, mix), "proof_bytes": len(distinct[0]), "distinct_proofs": len(set(distinct)), "device": {}, "kernels_ms": {}}
    biggest = max(batches)
    proofs = [distinct[i % 8] for i in range(biggest)]
    for n in batches:
        batch = proofs[:n]
        buf = np.frombuffer(b"".join(batch), dtype=np.uint8)
        off = np.arange(n + 1, dtype=np.uintp) * len(batch[0])
        rep = (ctypes.c_uint32 * (4 * n))()

        def call(handle):
            t0 = time.perf_counter()
            rc = lib.p2gpu_verify_batch(handle, buf.ctypes.data, off.ctypes.data, n, ctypes.byref(rep))
            dt = time.perf_counter() - t0
            assert rc == 0, lib.p2gpu_last_error()
            return dt

        w = windowed(lambda: call(vd._h), window)
        w["proofs_per_s"] = round(n / (w["ms"] * 1e-3), 1)
        out["device"][str(n)] = w
        cd.set("profile", 2)
        cd.kernel_stats()
        call(cd._h)
        ks = cd.kernel_stats()
        cd.set("profile", 0)
        out["kernels_ms"][str(n)] = {k: round(v["ms"], 3) for k, v in ks.items() if k.startswith("verify_")}
    n1 = min(biggest, 64)
    h1 = windowed(lambda: host_loop(lib, vd._h, proofs[:n1], 1), window, warm=1)
    h16 = windowed(lambda: host_loop(lib, vd._h, proofs, 16), window, warm=1)
    h1.update(proofs=n1, proofs_per_s=round(n1 / (h1["ms"] * 1e-3), 1))
    h16.update(proofs=biggest, proofs_per_s=round(biggest / (h16["ms"] * 1e-3), 1))
    out["host"] = {"threads_1": h1, "threads_16": h16, "cpus": len(os.sched_getaffinity(0))}
    top = out["device"][str(biggest)]["proofs_per_s"]
    out["device_over_16_threads_at_%d" % biggest] = round(top / out["host"]["threads_16"]["proofs_per_s"], 2)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--circuits", default="13:arith,17:sha")
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back calls behind every figure")
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(",")]
    if a.child:
        d, mix = a.child.split(":")
        return measure(int(d), mix, batches, a.window)
    results = []
    for spec in a.circuits.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", spec, "--batches", a.batches, "--window", str(a.window)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:  # a step that fails or runs out of time ends the measurement: nothing more is started on the GPU
            sys.stderr.write(r.stderr[-2000:])
            print(json.dumps({"error": "step %s ended with status %d" % (spec, r.returncode), "results": results}))
            return 1
        results.append(json.loads(r.stdout.strip().split("\n")[-1]))
    print(json.dumps({"verify_batch": results}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
