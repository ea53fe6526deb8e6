"""solver's values -> proof, two ways in one process, alternating:
  (a) the parent path: translate.py's build() event loop on the host, then p2gpu_prove from the host matrix;
  (b) p2gpu_prove_seeds: the witness plan's level walk on the device, then the resident proof;
and p2gpu_prove_dev alone on the resident matrix (the floor (b) can approach).  Also the plan's compile time and level-walk
kernel time for the SHA-256 compression circuit and the reference's basic_if / basic_div, and four proofs in flight on four
handles through prove_seeds against prove_dev.
usage: witness_time.py [runs] [inflight_seconds]   -- one JSON line on stdout."""
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import __graft_entry__ as entry  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
import gen_proof_digests as gen  # noqa: E402
import test_translate  # noqa: E402

pkg = entry.load_package()
runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
inflight_s = float(sys.argv[2]) if len(sys.argv) > 2 else 3.0
SHA = [("sha256_compression", list(range(16)), list(range(16, 24)), list(range(24, 32)))]
WIT = {i: v for i, v in enumerate([1 << 31] + [0] * 15 + gen.SHA256_IV)}


def stats(x):
    return {"median": statistics.median(x), "min": min(x), "max": max(x)}


def sha_builder():
    cb = pkg.translate.CircuitBuilderFromAcirToPlonky2()
    cb.translate_circuit(SHA)
    return cb


def plan_figures(cb, witness):
    cells, values = cb.witness_seeds(witness)
    cd = pkg.CircuitData(cb.blob())
    plan = cd.witness_plan(cells)
    walks = []
    for _ in range(runs + 1):
        plan.generate(values)
        walks.append(plan.info()["walk_ms"])
    info = plan.info()
    info["walk_ms"] = stats(walks[1:])
    info["walk_us_per_level"] = 1e3 * info["walk_ms"]["median"] / info["levels"]
    plan.close()
    cd.close()
    return info


res = {"runs": runs, "plans": {}}
for name, prog in test_translate._reference_programs().items():
    cb = pkg.translate.CircuitBuilderFromAcirToPlonky2(num_wires=135)
    cb.translate_circuit(prog["opcodes"], public_parameters=prog["public"], private_parameters=prog["private"])
    res["plans"][name] = plan_figures(cb, prog["witness"])
res["plans"]["sha256_compression"] = plan_figures(sha_builder(), WIT)

# ---- lone proof: (a) event loop + p2gpu_prove, (b) p2gpu_prove_seeds, floor: p2gpu_prove_dev ----
cb = sha_builder()
cells, values = cb.witness_seeds(WIT)
blob = cb.blob()
cd = pkg.CircuitData(blob)
plan = cd.witness_plan(cells)
loop_ms, a_ms, b_ms, dev_ms = [], [], [], []
wires_dev = plan.generate(values).clone()
for i in range(runs + 1):
    fresh = sha_builder()          # (translation is the circuit's cost, not the witness's: outside the timed part)
    fresh.blob()
    t0 = time.perf_counter()
    _, wires = fresh.build(WIT)
    t1 = time.perf_counter()
    pa = cd.prove(wires)
    t2 = time.perf_counter()
    pb = plan.prove(values)
    t3 = time.perf_counter()
    pd = cd.prove(wires_dev)
    t4 = time.perf_counter()
    assert pa.to_bytes() == pb.to_bytes() == pd.to_bytes()
    if i:                          # (first round: warm-up)
        loop_ms.append((t1 - t0) * 1e3)
        a_ms.append((t2 - t0) * 1e3)
        b_ms.append((t3 - t2) * 1e3)
        dev_ms.append((t4 - t3) * 1e3)
res["lone_sha256"] = {"a_event_loop_ms": stats(loop_ms), "a_total_ms": stats(a_ms), "b_prove_seeds_ms": stats(b_ms), "prove_dev_ms": stats(dev_ms),
                      "walk_ms_last": plan.info()["walk_ms"]}
plan.close()
cd.close()

# ---- four proofs in flight on four handles ----
handles = [pkg.CircuitData(blob) for _ in range(4)]
plans = [h.witness_plan(cells) for h in handles]
mats = [p.generate(values).clone() for p in plans]


def rate(fn):
    counts = [0] * 4
    stop = time.perf_counter() + inflight_s

    def work(k):
        while time.perf_counter() < stop:
            fn(k)
            counts[k] += 1

    th = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    return sum(counts) / (time.perf_counter() - t0)


seeds_rate, dev_rate = [], []
for _ in range(3):
    dev_rate.append(rate(lambda k: handles[k].prove(mats[k])))
    seeds_rate.append(rate(lambda k: plans[k].prove(values)))
res["inflight4_sha256"] = {"prove_dev_per_s": stats(dev_rate), "prove_seeds_per_s": stats(seeds_rate)}
for p in plans:
    p.close()
for h in handles:
    h.close()
print(json.dumps(res))
