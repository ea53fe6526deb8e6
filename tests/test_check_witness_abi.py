"""The witness check's public surface, without a device: p2gpu_check_witness / p2gpu_check_witness_dev / p2gpu_check_seeds in the
library and the header, the report's layout as the C compiler and ctypes see it, the refusals that need no device, and the
Python entry points."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

E_ARG = -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "p2gpu.h")) as f:
        return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))


def test_symbols_and_header_signatures(pkg):
    lib = pkg.load_library()
    for name in ("p2gpu_check_witness", "p2gpu_check_witness_dev", "p2gpu_check_seeds"):
        assert hasattr(lib, name), name
    flat = _header()
    assert ("int p2gpu_check_witness_dev(p2gpu_circuit *c, const uint64_t *wires_dev, size_t batch, const uint64_t *public_inputs , "
            "uint32_t n_pi, p2gpu_witness_report *reports , uint16_t *row_status , uint8_t *cell_flags );") in flat
    assert ("int p2gpu_check_witness(p2gpu_circuit *c, const uint64_t *wires , const uint64_t *public_inputs, uint32_t n_pi, "
            "p2gpu_witness_report *report, uint16_t *row_status, uint8_t *cell_flags);") in flat
    assert ("int p2gpu_check_seeds(p2gpu_witness_plan *p, const uint64_t *seed_values, const uint64_t *public_inputs, uint32_t n_pi, "
            "p2gpu_witness_report *report, uint16_t *row_status, uint8_t *cell_flags);") in flat
    assert ("typedef struct { uint64_t gate_rows_failed; uint64_t copy_cells_failed; uint64_t noncanonical_cells; uint32_t gate_row, "
            "gate_index, gate_kind, constraint; uint64_t constraint_value; uint32_t copy_cell[2], copy_partner[2]; uint64_t "
            "copy_values[2]; uint32_t noncanonical_cell[2]; } p2gpu_witness_report;") in flat


def test_report_layout_matches_the_c_compiler(pkg, tmp_path):
    rep = pkg.prover._WitnessReport
    fields = [name for name, _ in rep._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "p2gpu.h"\nint main(void) {\n  printf("%zu", sizeof(p2gpu_witness_report));\n'
                   + "".join('  printf(" %%zu", offsetof(p2gpu_witness_report, %s));\n' % f for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == ctypes.sizeof(rep) == 88
    assert got[1:] == [getattr(rep, f).offset for f in fields]


def test_null_and_empty_batch_need_no_device(pkg):
    lib = pkg.load_library()
    rep = (pkg.prover._WitnessReport * 1)()
    one = ctypes.c_void_p(8)                      # (never dereferenced: the handle is refused first)
    assert lib.p2gpu_check_witness_dev(None, one, 1, None, 0, rep, None, None) == E_ARG
    assert lib.p2gpu_check_witness_dev(None, None, 0, None, 0, None, None, None) == E_ARG
    assert lib.p2gpu_check_witness(None, one, None, 0, rep, None, None) == E_ARG
    assert lib.p2gpu_check_seeds(None, None, None, 0, rep, None, None) == E_ARG


def test_verifier_only_handle_is_refused_without_a_device(pkg):
    """A verifier-only handle is made without touching a device (cap and digest are not looked at until a proof is): the
    refusals of a real handle -- null matrix, null reports, batch 0, the handle itself with its words -- can be seen here."""
    blob, _ = pkg.make_circuit(8, "ecdsa", seed=1)
    h = blob[:256].copy().view(np.uint32)
    ng, R, cap_h = int(h[23]), int(h[4]), int(h[10])
    h[25] = 3                                     # (flags: digest and cap present; both zero here)
    vk = h.tobytes() + blob[256:256 + 48 * ng].tobytes() + bytes(32 << cap_h) + blob[256 + 48 * ng:256 + 48 * ng + 8 * R].tobytes()
    vd = pkg.VerifierCircuitData(vk)
    try:
        lib, rep, one = pkg.load_library(), (pkg.prover._WitnessReport * 1)(), ctypes.c_void_p(8)
        assert lib.p2gpu_check_witness_dev(vd._h, None, 1, None, 0, rep, None, None) == E_ARG
        assert lib.p2gpu_check_witness_dev(vd._h, one, 0, None, 0, rep, None, None) == E_ARG
        assert lib.p2gpu_check_witness_dev(vd._h, one, 1, None, 0, None, None, None) == E_ARG
        assert lib.p2gpu_check_witness_dev(vd._h, one, 1, None, 0, rep, None, None) == E_ARG
        assert b"verifier-only" in lib.p2gpu_last_error()
        assert lib.p2gpu_check_witness(vd._h, one, None, 0, rep, None, None) == E_ARG
        assert b"verifier-only" in lib.p2gpu_last_error()
    finally:
        vd.close()


def test_python_entry_points(pkg):
    sig = inspect.signature(pkg.prover.CircuitData.check_witness)
    assert list(sig.parameters)[1:] == ["wires", "public_inputs", "details"]
    assert sig.parameters["public_inputs"].default == () and sig.parameters["details"].default is False
    sig = inspect.signature(pkg.prover.WitnessPlan.check)
    assert list(sig.parameters)[1:3] == ["values", "public_inputs"] and sig.parameters["public_inputs"].default == ()
    sig = inspect.signature(pkg.prover.WitnessPlan.check_batch)
    assert list(sig.parameters)[1:3] == ["values_list", "public_inputs"] and sig.parameters["public_inputs"].default is None
    assert pkg.WitnessReport is pkg.prover.WitnessReport
    raw = pkg.prover._WitnessReport()
    raw.gate_row = raw.gate_index = raw.gate_kind = raw.constraint = 0xFFFFFFFF
    rep = pkg.WitnessReport(raw)
    assert rep.ok and rep.first_gate is None and rep.first_copy is None and rep.first_noncanonical is None and rep.row_status is None
    raw.gate_rows_failed, raw.gate_row, raw.gate_index, raw.gate_kind, raw.constraint, raw.constraint_value = 2, 3, 6, 9, 2, 5
    rep = pkg.WitnessReport(raw)
    assert not rep.ok and rep.first_gate == (3, 6, 9, 2, 5)
    assert callable(pkg.translate.CircuitBuilder.explain) and callable(pkg.translate.CircuitBuilderFromAcirToPlonky2.explain)
