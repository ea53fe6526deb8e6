"""BlackBoxFuncCall::EcdsaSecp256k1 from program bytes to a circuit, without a GPU: acir.to_translator_opcodes on a program
written by acir.serialize_program (no reference-produced ACIR bytes exist), translate.EcdsaSecp256k1Translator on it, and build()
for the 160 bytes of the reference's ecdsa_secp256k1/Prover.toml.  The expected output comes from the integer model of
tests/curve_inputs.py, which reads the bytes as the reference reads them (little-endian per 32-byte string) and compares with
<=.  The circuit is built once per module: the host build, about 2^17 rows, is what this file's time is."""
import pytest

import curve_inputs as ci


@pytest.fixture(scope="module")
def program(pkg):
    circuit, witness = ci.ecdsa_program()
    prog = pkg.acir.deserialize_program(pkg.acir.serialize_program([circuit]))
    return prog["functions"][0], witness


def test_to_translator_opcodes(pkg, program):
    circuit, _ = program
    ops = pkg.acir.to_translator_opcodes(circuit)
    assert [op[0] for op in ops] == ["ecdsa_secp256k1", "assert_zero"]
    _, pkx, pky, signature, hashed_message, output = ops[0]
    assert (pkx, pky, signature, hashed_message, output) == (list(range(32, 64)), list(range(64, 96)), list(range(96, 160)), list(range(32)), 160)
    assert ops[1] == ("assert_zero", [], [(1, 160)], ci.GOLDILOCKS - 1)
    r1 = {"name": "EcdsaSecp256r1", **{k: v for k, v in ci.ecdsa_program()[0]["opcodes"][0][1].items() if k != "name"}}
    prog = pkg.acir.deserialize_program(pkg.acir.serialize_program([{"opcodes": [("BlackBoxFuncCall", r1)]}]))
    with pytest.raises(NotImplementedError, match="EcdsaSecp256r1"):
        pkg.acir.to_translator_opcodes(prog["functions"][0])


def test_the_model_on_the_prover_toml_values():
    """What DESIGN.md 2 says of the reference's test: under the reference's reading the public key is off the curve and
    R.x != r, but r <= R.x holds, so the output is 1; read big-endian the same bytes are a valid signature, R.x == r."""
    v = ci.prover_toml_bytes()
    args = (v["pub_key_x"], v["pub_key_y"], v["signature"], v["hashed_message"])
    r, big_r, out = ci.ecdsa_model(*args)
    assert not ci.on_curve((ci.ecdsa_reading(v["pub_key_x"]), ci.ecdsa_reading(v["pub_key_y"]))) and big_r[0] != r and r <= big_r[0] and out == 1
    big = lambda b: int.from_bytes(bytes(b), "big")  # noqa: E731
    r, big_r, out = ci.ecdsa_model(*args, reading=big)
    assert ci.on_curve((big(v["pub_key_x"]), big(v["pub_key_y"]))) and big_r[0] % ci.N == r and out == 1


@pytest.fixture(scope="module")
def translated(pkg, program):
    circuit, witness = program
    tr = pkg.translate.CircuitBuilderFromAcirToPlonky2()
    tr.translate_circuit(pkg.acir.to_translator_opcodes(circuit), circuit["public_parameters"], circuit["private_parameters"])
    return tr, witness


def test_the_translated_circuit_builds_with_the_models_output(pkg, translated):
    tr, witness = translated
    v = ci.prover_toml_bytes()
    r, big_r, out = ci.ecdsa_model(v["pub_key_x"], v["pub_key_y"], v["signature"], v["hashed_message"])
    assert out == 1
    blob, wires = tr.build(dict(witness))              # (the output is the circuit's to derive)
    assert tr.witness_value(ci.ECDSA_OUTPUT) == out
    assert wires.shape == (234, 1 << 17)               # measured: 98 626 gate rows
    b = tr.builder
    kinds = [g[0] for g in b.generators()]
    assert kinds.count("glv_decompose") == 2 and kinds.count("equality") == 128 and kinds[:3] == ["nonnative_inv", "nonnative_mul", "nonnative_mul"]
    assert sum(1 for row in b.rows if row["kind"] == "basesum" and row["base"] == 4) == 16 and not any(row["kind"] == "basesum" and row["base"] == 2 for row in b.rows)
    # the seeds of the device witness: the 160 bytes and the PublicInputGate row's wires, nothing else
    cells, values = tr.witness_seeds(witness)
    assert len(cells) == 160 + 230 and values[:160] == [witness[i] for i in range(160)]
    with pytest.raises(ValueError, match="unsatisfiable|contradicts"):
        tr.build({**witness, ci.ECDSA_OUTPUT: 0})
