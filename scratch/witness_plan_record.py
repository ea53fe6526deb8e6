"""Records the host plan compiler's output for the inputs of tests/witness_plan_recorded.py (profiles/witness_refactor.md):
p2gpu_witness_plan_create + WitnessPlan.export() on the GPU, per case the three arrays and the five counts; for the SHA-256
compression plan the counts and the SHA-256 digest of each array.
usage: witness_plan_record.py OUT.npz [--tree DIR]     (--tree: the built checkout whose library makes the recording)"""
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else HERE
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.join(HERE, "tests", "golden"))
import __graft_entry__ as entry  # noqa: E402
import numpy as np  # noqa: E402
import witness_plan_recorded as wpr  # noqa: E402

pkg = entry.load_package()
out = {}
for name, (blob, cells) in wpr.cases(pkg).items():
    cd = pkg.CircuitData(blob)
    plan = cd.witness_plan(cells)  # (the host compiler)
    info = plan.info()
    out[name + "/counts"] = np.array([info[k] for k in wpr.COUNTS], dtype=np.uint64)
    for field, a in zip(wpr.ARRAYS, plan.export()):
        if name in wpr.DIGEST_ONLY:
            out[name + "/" + field + "_sha256"] = np.array(wpr.digest(a))
        else:
            out[name + "/" + field] = np.ascontiguousarray(a).reshape(-1)
    print(name, {k: info[k] for k in wpr.COUNTS}, file=sys.stderr)
    plan.close()
    cd.close()
np.savez_compressed(sys.argv[1], **out)
print("wrote", sys.argv[1], os.path.getsize(sys.argv[1]), "bytes")
