"""inputs in host memory -> prover handle ready, two ways in one process, alternating:
  (a) p2gpu_build_blob (host, one thread) then p2gpu_circuit_create (upload + commitment);
  (b) p2gpu_circuit_build (upload of gate rows and copy pairs, everything else on the device).
usage: build_time.py <degree_bits> <mix> [runs]   -- one JSON line on stdout; P2GPU_TRACE=1 adds the create marks of every run."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import __graft_entry__ as entry  # noqa: E402
import torch  # noqa: E402
import device_build_inputs as dbi  # noqa: E402

pkg = entry.load_package()
d, mix = int(sys.argv[1]), sys.argv[2]
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
blob = pkg.make_circuit(d, mix, 1)[0]
kw = dbi.decompose(pkg, blob)
del blob


def path_a():
    t0 = time.perf_counter()
    b = pkg.build_blob(**kw)
    t1 = time.perf_counter()
    cd = pkg.CircuitData(b)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    cd.close()
    return (t2 - t0) * 1e3, (t1 - t0) * 1e3


def path_b():
    t0 = time.perf_counter()
    cd = pkg.CircuitData.build(**kw)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    cd.close()
    return (t1 - t0) * 1e3


path_a()
path_b()      # warm-up: code objects, the runtime's first allocations
a, host, b = [], [], []
for _ in range(runs):
    ta, th = path_a()
    a.append(ta)
    host.append(th)
    b.append(path_b())
res = {"circuit": f"synth({d}, {mix})", "routed_cells": kw["num_routed_wires"] << d, "copy_pairs": len(kw["copies"]), "runs": runs,
       "a_ms": {"median": statistics.median(a), "min": min(a), "max": max(a), "build_blob_median": statistics.median(host)},
       "b_ms": {"median": statistics.median(b), "min": min(b), "max": max(b)},
       "ratio_of_medians": statistics.median(a) / statistics.median(b), "slowest_b_below_fastest_a": max(b) < min(a)}
print(json.dumps(res))
