"""solver's values -> proof, two ways in one process, alternating:
  (a) the parent path: translate.py's build() event loop on the host, then p2gpu_prove from the host matrix;
  (b) p2gpu_prove_seeds: the witness plan's level walk on the device, then the resident proof;
and p2gpu_prove_dev alone on the resident matrix (the floor (b) can approach).  Also the plan's compile time and level-walk
kernel time for the SHA-256 compression circuit and the reference's basic_if / basic_div, and four proofs in flight on four
handles through prove_seeds against prove_dev.
Many witnesses in one walk (p2gpu_generate_witness_batch): `batch_sha256` -- one batch of B against B lone calls, walk and
whole call, B = 1 .. 64 -- and `inflight4_sha256.with_batch8` -- the four resident proofs in flight with a fifth handle
walking batches of 8 beside them.
usage: witness_time.py [runs] [inflight_seconds] [--only SECTION,...] [--tree DIR] [--against DIR] [--compile host|device]
       [--batch-sizes B,...]
  -- one JSON line on stdout.  SECTIONs: plans, sha_plan (the SHA-256 plan alone), lone, batch, inflight; default: all but
  sha_plan.
  --tree DIR     measure the package of another checkout of this repository (built there), with this script: an older
                 commit (sha_plan, plans, lone), or a build with another WALK_GROUP (batch).
  --against DIR  `--only sha_plan` in fresh processes, alternating between DIR and this checkout, `runs` times each: the lone
                 walk of two commits side by side.
  --compile HOW  which plan compiler makes every plan: host (p2gpu_witness_plan_create, the default) or device
                 (p2gpu_witness_plan_build).  `plans.*.compile_ms` is that compiler's time; for five alternating runs in fresh
                 processes call `--only sha_plan` (or `plans`) once per run and compiler.  P2GPU_TRACE=1 prints the device
                 compiler's per-phase marks on stderr.
  --batch-sizes  the B of `batch` (default 1,2,4,8,16,32,64)."""
import json
import os
import statistics
import subprocess
import sys
import threading
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv, opts = [], {}
it = iter(sys.argv[1:])
for arg in it:
    if arg in ("--only", "--tree", "--against", "--compile", "--batch-sizes"):
        opts[arg] = next(it)
    else:
        argv.append(arg)
runs = int(argv[0]) if argv else 5
inflight_s = float(argv[1]) if len(argv) > 1 else 3.0
ROOT = os.path.abspath(opts.get("--tree", HERE))
# (no keyword for the host compiler: an older checkout given as --tree has none)
PLAN_KW = {"compile": "device"} if opts.get("--compile", "host") == "device" else {}
assert opts.get("--compile", "host") in ("host", "device")
only = set(opts["--only"].split(",")) if "--only" in opts else {"plans", "lone", "batch", "inflight"}


def stats(x):
    return {"median": statistics.median(x), "min": min(x), "max": max(x)}


if "--against" in opts:
    trees = {"other": os.path.abspath(opts["--against"]), "this": HERE}
    walks = {k: [] for k in trees}
    for _ in range(runs):
        for k, tree in trees.items():
            line = subprocess.run([sys.executable, os.path.abspath(__file__), "3", "--only", "sha_plan", "--tree", tree], check=True,
                                  stdout=subprocess.PIPE, text=True).stdout.strip().splitlines()[-1]
            walks[k].append(json.loads(line)["plans"]["sha256_compression"]["walk_ms"]["median"])
    print(json.dumps({"runs": runs, "trees": trees, "lone_walk_ms": {k: dict(stats(v), each=v) for k, v in walks.items()}}))
    sys.exit(0)

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import __graft_entry__ as entry  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
import gen_proof_digests as gen  # noqa: E402
import test_translate  # noqa: E402

pkg = entry.load_package()
SHA = [("sha256_compression", list(range(16)), list(range(16, 24)), list(range(24, 32)))]
WIT = {i: v for i, v in enumerate([1 << 31] + [0] * 15 + gen.SHA256_IV)}


def sha_builder():
    cb = pkg.translate.CircuitBuilderFromAcirToPlonky2()
    cb.translate_circuit(SHA)
    return cb


def plan_figures(cb, witness):
    cells, values = cb.witness_seeds(witness)
    cd = pkg.CircuitData(cb.blob())
    plan = cd.witness_plan(cells, **PLAN_KW)
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


res = {"runs": runs, "tree": ROOT, "compile": opts.get("--compile", "host"), "plans": {}}
if "plans" in only:
    for name, prog in test_translate._reference_programs().items():
        cb = pkg.translate.CircuitBuilderFromAcirToPlonky2(num_wires=135)
        cb.translate_circuit(prog["opcodes"], public_parameters=prog["public"], private_parameters=prog["private"])
        res["plans"][name] = plan_figures(cb, prog["witness"])
if only & {"plans", "sha_plan"}:
    res["plans"]["sha256_compression"] = plan_figures(sha_builder(), WIT)
if not only & {"lone", "batch", "inflight"}:
    print(json.dumps(res))
    sys.exit(0)

cb = sha_builder()
cells, values = cb.witness_seeds(WIT)
blob = cb.blob()

# ---- lone proof: (a) event loop + p2gpu_prove, (b) p2gpu_prove_seeds, floor: p2gpu_prove_dev ----
cd = pkg.CircuitData(blob)
plan = cd.witness_plan(cells, **PLAN_KW)
loop_ms, a_ms, b_ms, dev_ms = [], [], [], []
wires_dev = plan.generate(values).clone()
for i in range(runs + 1 if "lone" in only else 0):
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
if "lone" in only:
    res["lone_sha256"] = {"a_event_loop_ms": stats(loop_ms), "a_total_ms": stats(a_ms), "b_prove_seeds_ms": stats(b_ms),
                          "prove_dev_ms": stats(dev_ms), "walk_ms_last": plan.info()["walk_ms"]}
del wires_dev


# ---- one batch of B against B lone calls, alternating: device time of the walk(s), and the whole call(s) to the last sync ----
def members(B):
    """B different blocks and states (member 0: WIT's) on the plan's seed set."""
    rng = np.random.default_rng(7)
    return [values] + [[int(x) for x in rng.integers(0, 1 << 32, size=24)] + values[24:] for _ in range(B - 1)]


if "batch" in only:
    res["batch_sha256"] = {}
    for B in [int(b) for b in opts.get("--batch-sizes", "1,2,4,8,16,32,64").split(",")]:
        vals = members(B)
        fig = {k: [] for k in ("batch_walk_ms", "batch_call_ms", "lone_walk_ms", "lone_call_ms")}
        for i in range(runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, status, _ = plan.generate_batch(vals)
            t1 = time.perf_counter()
            bw = plan.info()["walk_ms"]
            assert status == [0] * B
            last = out[B - 1].clone()
            del out
            lw = 0.0
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            for v in vals:
                m = plan.generate(v)
                lw += plan.info()["walk_ms"]
            t3 = time.perf_counter()
            assert torch.equal(m, last)
            del m, last
            if i:                  # (first round: warm-up, and the plan's batched buffers grow)
                for k, x in zip(fig, (bw, (t1 - t0) * 1e3, lw, (t3 - t2) * 1e3)):
                    fig[k].append(x)
        r = {k: stats(x) for k, x in fig.items()}
        r["walk_ms_per_witness"] = {"batch": r["batch_walk_ms"]["median"] / B, "lone": r["lone_walk_ms"]["median"] / B}
        r["call_ms_per_witness"] = {"batch": r["batch_call_ms"]["median"] / B, "lone": r["lone_call_ms"]["median"] / B}
        res["batch_sha256"][str(B)] = r
plan.close()
cd.close()
if "inflight" not in only:
    print(json.dumps(res))
    sys.exit(0)

# ---- four proofs in flight on four handles ----
handles = [pkg.CircuitData(blob) for _ in range(4)]
plans = [h.witness_plan(cells, **PLAN_KW) for h in handles]
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

# ---- the same four resident proofs, with and without a fifth handle walking batches of 8 beside them ----
side_cd = pkg.CircuitData(blob)
side_plan = side_cd.witness_plan(cells, **PLAN_KW)
side_vals = members(8)
side_plan.generate_batch(side_vals)
alone, beside, batches = [], [], []
for _ in range(3):
    alone.append(rate(lambda k: handles[k].prove(mats[k])))
    done, count = threading.Event(), [0]

    def walk():
        while not done.is_set():
            side_plan.generate_batch(side_vals)
            count[0] += 1

    th = threading.Thread(target=walk)
    t0 = time.perf_counter()
    th.start()
    beside.append(rate(lambda k: handles[k].prove(mats[k])))
    done.set()
    th.join()
    batches.append(count[0] / (time.perf_counter() - t0))
res["inflight4_sha256"]["with_batch8"] = {"prove_dev_per_s_alone": stats(alone), "prove_dev_per_s_beside": stats(beside),
                                         "batches_of_8_per_s": stats(batches)}
side_plan.close()
side_cd.close()
for p in plans:
    p.close()
for h in handles:
    h.close()
print(json.dumps(res))
