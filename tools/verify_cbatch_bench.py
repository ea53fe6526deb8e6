#!/usr/bin/env python3
"""Compressed proofs per second of p2gpu_verify_batch_compressed on the GPU beside the two ways there were before it, same
proofs, same machine: (2) a loop of p2gpu_verify_compressed on 16 host threads, (3) p2gpu_proof_decompress on 16 host threads
followed by one p2gpu_verify_batch over the decompressed bytes.  Prints one JSON line.

    python tools/verify_cbatch_bench.py [--circuits 13:arith,17:sha] [--batches 1,64,1024] [--window 0.5] [--step-timeout 300]

Each circuit is measured in a child process of its own under `timeout`: it proves the synthetic circuit on the GPU -- eight
witnesses that differ in a free wire cell, repeated up to the batch size --, compresses the proofs, and times the three ways at
every batch size; then one more device call with the handle's "profile" knob (2: every launch) for the times of the kernels.
A figure is never one call: after two warm-up calls the same call is repeated back to back until --window seconds have passed
(five calls at least), and the median, the fastest and the slowest call are reported; proofs per second are taken from the
median."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from verify_batch_bench import P, windowed  # noqa: E402

THREADS = 16


def on_threads(work, items):
    """seconds for work(item) over the items, dealt round-robin to THREADS threads (ctypes releases the interpreter lock)"""
    def run(k):
        for it in items[k::THREADS]:
            work(it)

    ts = [threading.Thread(target=run, args=(k,)) for k in range(THREADS)]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return time.perf_counter() - t0


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
    want = len(distinct[0])
    compressed = [vd.compress(p) for p in distinct]
    out = {"circuit": "synth(%d, %s)" % (d, mix), "proof_bytes": want, "compressed_bytes": [len(c) for c in compressed],
           "distinct_proofs": len(set(distinct)), "device": {}, "host_threads_16": {}, "host_decompress_then_device": {}, "kernels_ms": {},
           "upload_bytes": {}, "cpus": len(os.sched_getaffinity(0))}
    for n in batches:
        batch = [compressed[i % 8] for i in range(n)]
        bufs = [np.frombuffer(c, dtype=np.uint8) for c in batch]
        buf = np.frombuffer(b"".join(batch), dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.uintp)
        off[1:] = np.cumsum([len(c) for c in batch], dtype=np.uint64)
        rep = (ctypes.c_uint32 * (4 * n))()
        plain = np.zeros((n, want), dtype=np.uint8)
        plain_off = np.arange(n + 1, dtype=np.uintp) * want
        bad = []

        def device(handle):
            t0 = time.perf_counter()
            rc = lib.p2gpu_verify_batch_compressed(handle, buf.ctypes.data, off.ctypes.data, n, ctypes.byref(rep))
            dt = time.perf_counter() - t0
            assert rc == 0, lib.p2gpu_last_error()
            return dt

        def lone(i):
            if lib.p2gpu_verify_compressed(vd._h, bufs[i].ctypes.data, bufs[i].size):
                bad.append(i)

        def decompress(i):
            ln = ctypes.c_size_t(want)
            if lib.p2gpu_proof_decompress(vd._h, bufs[i].ctypes.data, bufs[i].size, plain[i].ctypes.data, ctypes.byref(ln)):
                bad.append(i)

        def decompress_then_device():
            t0 = time.perf_counter()
            on_threads(decompress, list(range(n)))
            rc = lib.p2gpu_verify_batch(vd._h, plain.ctypes.data, plain_off.ctypes.data, n, ctypes.byref(rep))
            dt = time.perf_counter() - t0
            assert rc == 0, lib.p2gpu_last_error()
            return dt

        for key, call in (("device", lambda: device(vd._h)), ("host_threads_16", lambda: on_threads(lone, list(range(n)))),
                          ("host_decompress_then_device", decompress_then_device)):
            w = windowed(call, window)
            w["proofs_per_s"] = round(n / (w["ms"] * 1e-3), 1)
            out[key][str(n)] = w
        assert not bad, "the host rejected a proof"
        cd.set("profile", 2)
        cd.kernel_stats()
        device(cd._h)
        ks = cd.kernel_stats()
        cd.set("profile", 0)
        out["kernels_ms"][str(n)] = {k: round(v["ms"], 3) for k, v in ks.items() if k.startswith(("verify_", "decompress_"))}
        out["upload_bytes"][str(n)] = {"compressed": int(off[-1]), "uncompressed": n * want}
    top = str(max(batches))
    out["device_over_host_threads_16_at_" + top] = round(out["host_threads_16"][top]["ms"] / out["device"][top]["ms"], 2)
    out["device_over_host_decompress_then_device_at_" + top] = round(out["host_decompress_then_device"][top]["ms"] / out["device"][top]["ms"], 2)
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
    print(json.dumps({"verify_batch_compressed": results}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
