"""The circuits whose host-compiled witness plan is recorded under tests/golden/ (test infrastructure): every input of
tests/test_gpu_witness_plan.py's plan-equality tests as (circuit blob, seed cells), made on the CPU.  The recording itself
(witness_plans.npz: per case cell_slot, ops, level_off and the five counts; the SHA-256 compression plan as counts and
digests only) comes from p2gpu_witness_plan_create on the MI355X at the commit before the host compiler moved to
csrc/planhost.hpp -- scratch/witness_plan_record.py wrote it, profiles/witness_refactor.md has the recipe."""
import hashlib
import os

import numpy as np

import witness_gen_inputs as wgi
import witness_plan_inputs as wpi

COUNTS = ("ops", "levels", "widest_level", "slots", "seeds")
ARRAYS = ("cell_slot", "ops", "level_off")
DIGEST_ONLY = ("sha256_compression",)  # cell_slot alone is 10 MB


def sha256_case(pkg):
    import gen_proof_digests as gen

    cb = wgi.translated(pkg, dict(opcodes=[("sha256_compression", list(range(16)), list(range(16, 24)), list(range(24, 32)))]))
    wit = {i: v for i, v in enumerate([1 << 31] + [0] * 15)}
    wit.update({16 + i: v for i, v in enumerate(gen.SHA256_IV)})
    cells, _ = cb.witness_seeds(wit)
    return cb.blob(), cells


def cases(pkg):
    """{name: (blob, seed cells)} in the recording's order."""
    import test_translate

    out = {}
    for name in sorted(wpi.HAND_BUILT):
        kw, cells = wpi.HAND_BUILT[name]()
        out[name] = (pkg.build_blob(**kw), cells)
    for name, prog in (("fibonacci", wgi.FIBONACCI), ("quadratic", wgi.QUADRATIC), ("bitwise", wgi.BITWISE)):
        cb = wgi.translated(pkg, prog)
        blob, _ = cb.build(prog["witness"])
        out[name] = (blob, cb.builder.seed_cells())
    kw, cells, _, _ = wgi.custom_gate_chain()
    out["custom_gate_chain"] = (pkg.build_blob(**kw), cells)
    for name in ("basic_if", "basic_div"):
        prog = test_translate._reference_programs()[name]
        cb = wgi.translated(pkg, prog, num_wires=135, public_parameters=prog["public"], private_parameters=prog["private"])
        out[name] = (cb.blob(), cb.builder.seed_cells())
    out["sha256_compression"] = sha256_case(pkg)
    return out


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load(golden):
    """{name: {"counts": [5], and per array either the array or "<array>_sha256"}}"""
    z = np.load(os.path.join(golden, "witness_plans.npz"))
    out = {}
    for key in z.files:
        name, field = key.split("/")
        out.setdefault(name, {})[field] = z[key]
    return out


def compare(name, rec, counts, arrays):
    """counts: the five in COUNTS' order; arrays: cell_slot (flat or [R][n]), ops, level_off.  Byte for byte."""
    assert [int(x) for x in rec["counts"]] == [int(x) for x in counts], (name, rec["counts"], counts)
    for field, a in zip(ARRAYS, arrays):
        a = np.ascontiguousarray(a).reshape(-1)
        if field in rec:
            want = rec[field]
            assert a.dtype == want.dtype and a.shape == want.shape, (name, field, a.dtype, a.shape, want.shape)
            bad = np.flatnonzero(a != want)
            assert bad.size == 0, (name, field, len(bad), bad[:4].tolist(), a[bad[:4]].tolist(), want[bad[:4]].tolist())
        else:
            assert digest(a) == str(rec[field + "_sha256"]), (name, field)
