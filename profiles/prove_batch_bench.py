#!/usr/bin/env python3
"""Proofs per second of p2gpu_prove_batch_dev against the two ways a caller had before it, on one MI355X, in one session:

  batch   one p2gpu_prove_batch_dev call over B resident witnesses of the `arith` mix
  loop    the same witnesses through p2gpu_prove_dev one after the other on the same handle (WitnessPlan.prove_batch's loop)
  four    four handles of the circuit on four threads, each proving its quarter alone (tests/in_flight.py)

The three are run alternately, REPS times after one warm-up round; the table gives the median and the spread (min .. max) of
the proofs per second.  Every proof of the first round is compared with the lone proof's bytes.  Also recorded: the launches
of a slab, the registers and scratch of each kernel (from a compiler resource report: --resource-log, a file made with
`hipcc ... -Rpass-analysis=kernel-resource-usage -c provebatch.hip`; without it that compile runs here), and the share of
each kernel in one profiled batch call (knob profile = 2) in a run of its own.  Writes profiles/prove_batch.md (--out).

Stand-alone: python profiles/prove_batch_bench.py [--degrees 3,5,8,10,12] [--batch 256] [--reps 5]"""
import os
import sys

# (run as a script, this directory leads sys.path, and its numbers.py would stand in for the standard library's)
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != os.path.dirname(os.path.abspath(__file__))]

import argparse  # noqa: E402
import ctypes  # noqa: E402
import re  # noqa: E402
import statistics  # noqa: E402
import subprocess  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import in_flight  # noqa: E402
import witness_gen_inputs as wgi  # noqa: E402

CSRC = os.path.join(ROOT, "acvm-backend-plonky2_amd", "csrc")


def resource_table(log_path):
    if log_path:
        with open(log_path) as f:
            text = f.read()
    else:
        cmd = ["hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-Wno-pass-failed", "-Wno-inline-asm",
               "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "provebatch.hip"), "-o", os.devnull]
        text = subprocess.run(cmd, capture_output=True, text=True).stderr
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip() or m.group(1)
            m2 = re.search(r"pb::(\w+)(<\d>)?", name)
            cur = {"name": (m2.group(1) + (m2.group(2) or "")) if m2 else name}
            rows.append(cur)
            continue
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("sgpr", r"SGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return rows


def measure(pkg, d, batch, reps):
    import torch

    lib = pkg.load_library()
    if d >= 5:
        blob, wires = pkg.make_circuit(d, "arith", seed=1)
    else:                       # the workload generator starts at 2^5 gates: below it, the translated two-opcode program of the tests
        assert d == 3, "degree_bits 3 (tests/witness_gen_inputs.py QUADRATIC) or >= 5 (the arith mix)"
        cb = wgi.translated(pkg, wgi.QUADRATIC)
        blob, wires = cb.build(wgi.QUADRATIC["witness"])
        wires = np.ascontiguousarray(wires)
    handles = [pkg.CircuitData(blob) for _ in range(4)]
    cd = handles[0]
    one = torch.from_numpy(wires.view(np.int64)).to("cuda:0")
    stack = one.unsqueeze(0).repeat(batch, 1, 1).contiguous()
    torch.cuda.synchronize()
    lone = cd.prove(one).to_bytes()
    bound = cd._bound
    out = np.zeros((batch, bound), dtype=np.uint8)
    status = np.zeros(batch, dtype=np.intc)
    single = np.zeros(bound, dtype=np.uint8)

    def run_batch():
        t0 = time.perf_counter()
        rc = lib.p2gpu_prove_batch_dev(cd._h, ctypes.c_void_p(stack.data_ptr()), batch, None, 0, out.ctypes.data, status.ctypes.data)
        dt = time.perf_counter() - t0
        assert rc == 0, lib.p2gpu_last_error()
        return dt

    base, stride = stack.data_ptr(), 8 * wires.size

    def prove_alone(h, members, buf, check=False):
        plen = ctypes.c_size_t(0)
        for b in members:
            plen.value = bound
            rc = lib.p2gpu_prove_dev(h._h, ctypes.c_void_p(base + b * stride), None, 0, buf.ctypes.data, ctypes.byref(plen), None)
            assert rc == 0, lib.p2gpu_last_error()
            if check:
                assert buf.tobytes() == lone

    def run_loop(check=False):
        t0 = time.perf_counter()
        prove_alone(cd, range(batch), single, check)
        return time.perf_counter() - t0

    def run_four():
        bufs = [np.zeros(bound, dtype=np.uint8) for _ in range(4)]

        def worker(i, stop):
            plen = ctypes.c_size_t(0)
            for b in range(i, batch, 4):
                if stop.is_set():
                    return
                plen.value = bound
                rc = lib.p2gpu_prove_dev(handles[i]._h, ctypes.c_void_p(base + b * stride), None, 0, bufs[i].ctypes.data, ctypes.byref(plen), None)
                yield ("rc %d" % b, rc, 0)
            yield ("bytes", bufs[i].tobytes(), lone)

        t0 = time.perf_counter()
        in_flight.run_in_flight([in_flight.Worker(worker, len(range(i, batch, 4)) + 1, "prover %d" % i) for i in range(4)], 600)
        return time.perf_counter() - t0

    try:
        run_batch(), run_loop(check=True), run_four()      # warm-up: buffers, code objects; every proof's bytes looked at once
        assert all(out[b].tobytes() == lone for b in range(batch)) and not status.any()
        times = {"batch": [], "loop": [], "four": []}
        for _ in range(reps):
            times["batch"].append(run_batch())
            times["loop"].append(run_loop())
            times["four"].append(run_four())
        info = cd.prove_batch_info()
        # the per-kernel share, in a run of its own
        cd.set("profile", 2)
        run_batch()
        stats = cd.kernel_stats()
        cd.set("profile", 0)
        return {k: [batch / t for t in v] for k, v in times.items()}, info, {k: v for k, v in stats.items() if k.startswith("pb_")}
    finally:
        for h in handles:
            h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degrees", default="3,5,8,10,12")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resource-log", default=None)
    ap.add_argument("--build", action="store_true", help="run the build first (default: only when the library is missing)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prove_batch.md"))
    args = ap.parse_args()
    pkg = entry.load_package()
    if args.build or not os.path.exists(pkg.prover.lib_path()):
        entry.build()
    import torch

    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    lines = ["# p2gpu_prove_batch_dev against the lone-call loop and four proofs in flight", "",
             "Written by `profiles/prove_batch_bench.py` on %s; `arith` mix (degree_bits 3: the translated QUADRATIC program of the tests), %d resident witnesses per call, %d timed rounds after one"
             % (pkg.device_info()["name"], args.batch, args.reps),
             "warm-up round, the three paths alternating; proofs per second, median (min .. max).  Every proof of the warm-up round was",
             "compared with the lone proof's bytes.", "",
             "| degree_bits | batch call | lone-call loop | four in flight | winner | batch / loop | batch / four | launches per slab | proofs per slab |",
             "|---|---|---|---|---|---|---|---|---|"]
    shares, verdicts = {}, []
    for d in [int(x) for x in args.degrees.split(",")]:
        rates, info, stats = measure(pkg, d, args.batch, args.reps)
        med = {k: statistics.median(v) for k, v in rates.items()}
        cell = lambda k: "%.0f (%.0f .. %.0f)" % (med[k], min(rates[k]), max(rates[k]))   # noqa: E731
        lines.append("| %d | %s | %s | %s | %s | %.2f | %.2f | %d | %d |" % (d, cell("batch"), cell("loop"), cell("four"), max(med, key=med.get),
                                                                       med["batch"] / med["loop"], med["batch"] / med["four"], info["launches"], info["slab"]))
        shares[d] = stats
        verdicts.append("* degree_bits %d: %s wins; the batch call is %.2fx the loop and %.2fx four in flight"
                        % (d, max(med, key=med.get), med["batch"] / med["loop"], med["batch"] / med["four"]))
        print(lines[-1], flush=True)
    lines += ["", "## Which path wins (why: DESIGN.md 6d)", ""] + verdicts
    lines += ["", "## Share of each kernel in one batch call (knob `profile` = 2, HIP events around every launch, a run of its own)", "",
              "| kernel | " + " | ".join("d = %d" % d for d in shares) + " |", "|---|" + "---|" * len(shares)]
    names = sorted({k for s in shares.values() for k in s})
    for nm in names:
        row = []
        for d, s in shares.items():
            tot = sum(v["ms"] for v in s.values()) or 1.0
            row.append("%.1f %% (%.2f ms, %d)" % (100 * s[nm]["ms"] / tot, s[nm]["ms"], s[nm]["launches"]) if nm in s else "-")
        lines.append("| %s | %s |" % (nm, " | ".join(row)))
    lines.append("| all launches, ms | " + " | ".join("%.2f" % sum(v["ms"] for v in s.values()) for s in shares.values()) + " |")
    lines += ["", "## Registers and scratch of each kernel (compiler resource report, gfx950)", "",
              "| body | VGPRs | SGPRs | scratch bytes per lane | waves per SIMD |", "|---|---|---|---|---|"]
    for r in resource_table(args.resource_log):
        lines.append("| %s | %s | %s | %s | %s |" % (r["name"], r.get("vgpr", "?"), r.get("sgpr", "?"), r.get("scratch", "?"), r.get("occupancy", "?")))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
