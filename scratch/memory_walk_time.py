"""The device witness of a write-heavy memory circuit -- a 16-word block, 32 writes and 32 reads, every index the witness's
choice: 512 equality generators (one field inversion each, on one lane while the rest of its level waits at the barrier) -- by
scratch/witness_time.py's method: the plan's shape, compile_ms of both compilers, the level walk's device time lone and for a
batch of 8; and from the same run the walk of the SHA-256 compression circuit, an existing plan without such generators, as
the comparison.
usage: memory_walk_time.py [runs]   -- one JSON line on stdout"""
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests", "golden"))
import __graft_entry__ as entry  # noqa: E402
import numpy as np  # noqa: E402
import gen_proof_digests as gen  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
pkg = entry.load_package()
WORDS, STEPS, BATCH = 16, 32, 8


def stats(x):
    return {"median": statistics.median(x), "min": min(x), "max": max(x)}


def memory_program():
    """(opcodes, private parameters, witness): step t writes value w[+1] at w[+0], then reads w[+3] at w[+2]."""
    rng = np.random.default_rng(7)
    ops = [("memory_init", 0, list(range(WORDS)))]
    block = [int(v) for v in rng.integers(0, 1 << 32, size=WORDS)]
    witness = dict(enumerate(block))
    private = list(range(WORDS))
    for t in range(STEPS):
        w = WORDS + 4 * t
        i, v, j = (int(x) for x in rng.integers(0, WORDS, size=3))
        v = int(rng.integers(0, 1 << 32))
        ops += [("memory_op", 0, 1, w, w + 1), ("memory_op", 0, 0, w + 2, w + 3)]
        block[i] = v
        witness.update({w: i, w + 1: v, w + 2: j, w + 3: block[j]})
        private += [w, w + 1, w + 2]
    return ops, private, witness


def figures(cb, witness, compilers):
    cells, values = cb.witness_seeds(witness)
    gens = cb.witness_generators()
    cd = pkg.CircuitData(cb.blob())
    out = {"generators": len(gens), "degree_bits": int(np.log2(cd.degree)), "compile_ms": {}}
    for how in compilers:
        compile_ms = []
        for _ in range(runs):
            plan = cd.witness_plan(cells, compile=how, generators=gens or None)
            compile_ms.append(plan.info()["compile_ms"])
            plan.close()
        out["compile_ms"][how] = stats(compile_ms)
    plan = cd.witness_plan(cells, generators=gens or None)
    lone, batch = [], []
    for _ in range(runs + 1):
        plan.generate(values)
        lone.append(plan.info()["walk_ms"])
    for _ in range(runs + 1):
        _, status, _ = plan.generate_batch([values] * BATCH)
        assert not any(status)
        batch.append(plan.info()["walk_ms"])
    info = plan.info()
    out.update(ops=info["ops"], levels=info["levels"], widest_level=info["widest_level"], slots=info["slots"],
               walk_ms_lone=stats(lone[1:]), walk_ms_batch8=stats(batch[1:]))
    out["walk_us_per_level_lone"] = 1e3 * out["walk_ms_lone"]["median"] / info["levels"]
    plan.close()
    cd.close()
    return out


res = {"runs": runs}
ops, private, witness = memory_program()
cb = pkg.translate.CircuitBuilderFromAcirToPlonky2()
cb.translate_circuit(ops, private_parameters=private)
res["memory_16_words_32_writes_32_reads"] = figures(cb, witness, ("host", "device"))
cb = pkg.translate.CircuitBuilderFromAcirToPlonky2()
cb.translate_circuit([("sha256_compression", list(range(16)), list(range(16, 24)), list(range(24, 32)))])
res["sha256_compression"] = figures(cb, {i: v for i, v in enumerate([1 << 31] + [0] * 15 + gen.SHA256_IV)}, ("host",))
print(json.dumps(res))
