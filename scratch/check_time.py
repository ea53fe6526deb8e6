"""Device time of the witness check (p2gpu_check_witness_dev) beside the quotient phase of p2gpu_prove_dev on the same handle, in
the same run.  One JSON document on stdout (and in the file given as the second argument); profiles/check_witness.md holds the
figures of the run on record.

    python scratch/check_time.py [repeats] [out.json] [--no-opcode]

Per circuit: the matrix is resident; two warm-up checks; then `repeats` checks with the handle's knob "profile" = 2, which times
every launch with HIP events on the handle's stream.  The check's parts are its launches: canonicity, gate rows, PoseidonGate
rows, sigma decode (the sorted powers of w and the binary search per cell, host allocations between its launches included: the
events bracket the whole phase) and the compare.  `check_wall_ms` is the host's time around the whole call (scratch allocation,
the read-back and the synchronisation included).  Then `repeats` resident proofs with profiling off: `quotient_ms` of
p2gpu_timings.  Figures are median [min - max] over the repeats."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

PARTS = {"check_canon_kernel": "canonicity", "check_gates_kernel": "gate_rows", "check_poseidon_kernel": "poseidon_rows",
         "check_sigma_decode": "sigma_decode", "check_copies_kernel": "copy_compare"}


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def measure(pkg, label, blob, wires, pis, repeats):
    import numpy as np
    import torch

    cd = pkg.CircuitData(blob)
    dev = torch.from_numpy(np.ascontiguousarray(wires).view(np.int64)).to(f"cuda:{cd.device_index()}")
    for _ in range(2):
        assert cd.check_witness(dev, pis).ok
    parts, wall = {name: [] for name in PARTS.values()}, []
    for _ in range(repeats):
        cd.set("profile", 2)                      # (also clears the statistics)
        t0 = time.perf_counter()
        rep = cd.check_witness(dev, pis)
        wall.append((time.perf_counter() - t0) * 1e3)
        assert rep.ok
        stats = cd.kernel_stats()
        for k, name in PARTS.items():
            parts[name].append(stats[k]["ms"] if k in stats else 0.0)
    cd.set("profile", 0)
    cd.prove(dev, pis)
    quotient, total = [], []
    for _ in range(repeats):
        t = cd.prove(dev, pis).timings
        quotient.append(t["quotient_ms"])
        total.append(t["total_ms"])
    res = {"circuit": label, "rows": cd.degree,
           "check_device_ms": spread([sum(p[i] for p in parts.values()) for i in range(repeats)]), "check_wall_ms": spread(wall),
           "parts_ms": {k: spread(v) for k, v in parts.items()}, "prove_quotient_ms": spread(quotient), "prove_total_ms": spread(total)}
    cd.close()
    return res


def synthetic(pkg, d, mix, repeats, npi=0):
    out = pkg.make_circuit(d, mix, seed=7, num_public_inputs=npi)
    label = "make_circuit(%d, %r%s)" % (d, mix, ", num_public_inputs=%d" % npi if npi else "")
    return measure(pkg, label, out[0], out[1], [int(x) for x in out[2]] if npi else [], repeats)


def ecdsa_opcode(pkg, repeats):
    """The translated EcdsaSecp256k1 opcode (98 626 gate rows, 2^17) with build()'s matrix; the program is the tests' own."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import curve_inputs as ci

    circuit, witness = ci.ecdsa_program()
    circuit = pkg.acir.deserialize_program(pkg.acir.serialize_program([circuit]))["functions"][0]
    t0 = time.perf_counter()
    tr = pkg.translate.CircuitBuilderFromAcirToPlonky2()
    tr.translate_circuit(pkg.acir.to_translator_opcodes(circuit), circuit["public_parameters"], circuit["private_parameters"])
    blob, wires = tr.build(dict(witness))
    host = round(time.perf_counter() - t0, 1)
    res = measure(pkg, "the EcdsaSecp256k1 opcode, translated", blob, wires, tr.public_inputs(), repeats)
    res["host_translate_and_build_s"] = host
    return res


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    entry.build()
    pkg = entry.load_package()
    doc = {"device": pkg.device_info()["name"], "repeats": repeats,
           "circuits": [synthetic(pkg, 17, "ecdsa", repeats), synthetic(pkg, 17, "sha", repeats), synthetic(pkg, 17, "sha", repeats, npi=4)]}
    if "--no-opcode" not in sys.argv:
        doc["circuits"].append(ecdsa_opcode(pkg, repeats))
    text = json.dumps(doc, indent=1)
    print(text)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
