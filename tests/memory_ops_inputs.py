"""The circuits of the reference's tests/test_memory_operations.rs restated as data, and the ones added beyond it; shared by
tests/test_reference_memory_tests.py (oracle) and tests/test_gpu_memory_ops.py (MI355X)."""
P = 0xFFFFFFFF00000001


def init(block, witnesses):
    return ("memory_init", block, list(witnesses))


def read(block, index, value):
    return ("memory_op", block, 0, index, value)


def write(block, index, value):
    return ("memory_op", block, 1, index, value)


def az(linear, q_c):
    return ("assert_zero", [], linear, q_c % P)


# test_memory_operations.rs:229-276 _memory_simple_read_circuit
READ = dict(ops=[init(0, [0, 1]), read(0, 2, 3), az([(1, 0), (P - 1, 3)], 0)], public=[0, 1, 2])
# :278-361 _memory_simple_write_circuit
WRITE = dict(ops=[init(0, [0, 1]), write(0, 2, 3), az([(P - 1, 4)], 0), read(0, 4, 5), az([(1, 5)], -1), az([(P - 1, 6)], 1),
                  read(0, 6, 7), az([(P - 1, 7)], 11)], public=[0, 1, 2, 3])
# :183-227 _read_memory_of_length_3_circuit
LENGTH_3 = dict(ops=[init(0, [0, 1, 2]), read(0, 3, 4), az([(1, 4)], -5)], public=[0, 1, 2, 3])
# beyond the reference
LENGTH_1 = dict(ops=[init(0, [0]), read(0, 1, 2), az([(1, 2)], -7)], public=[0, 1])
LENGTH_5 = dict(ops=[init(0, [0, 1, 2, 3, 4]), read(0, 5, 6), az([(1, 6)], -44)], public=[0, 1, 2, 3, 4, 5])
# x[i] = v; then x[j] and x[k] are read, every index the witness's choice
WRITE_READ = dict(ops=[init(0, [0, 1, 2]), write(0, 3, 4), read(0, 5, 6), read(0, 7, 8)], public=[0, 1, 2, 3, 4, 5, 7])

# (name, program, witness assignment, expected public inputs)
CASES = [
    ("read_memory_operation", READ, {0: 0, 1: 0, 2: 1, 3: 0}, [0, 0, 1]),                                              # :10-36
    ("basic_memory_write", WRITE, {0: 10, 1: 11, 2: 0, 3: 1, 4: 0, 5: 1, 6: 1, 7: 11}, [10, 11, 0, 1]),                 # :39-79
    ("memory_blocks_with_irregular_size", LENGTH_3, {0: 5, 1: 10, 2: 11, 3: 0, 4: 5}, [5, 10, 11, 0]),                  # :82-117
    ("block_of_length_1", LENGTH_1, {0: 7, 1: 0}, [7, 0]),
    ("block_of_length_5", LENGTH_5, {0: 40, 1: 41, 2: 42, 3: 43, 4: 44, 5: 4}, [40, 41, 42, 43, 44, 4]),
    ("write_then_read_written_and_other", WRITE_READ, {0: 20, 1: 21, 2: 22, 3: 2, 4: 99, 5: 2, 7: 1}, [20, 21, 22, 2, 99, 2, 1]),
]
WRITE_READ_RESULTS = {6: 99, 8: 21}


def translated(pkg, prog, num_wires=234):
    cb = pkg.translate.CircuitBuilderFromAcirToPlonky2(num_wires=num_wires)
    cb.translate_circuit(prog["ops"], public_parameters=prog["public"])
    return cb


def is_equal_circuit(pkg):
    """:388-429: standard_recursion_config (135 wires), x, y virtual targets, is_equal(x, y).  (builder, x, y, equal)."""
    b = pkg.translate.CircuitBuilder(num_wires=135)
    x, y = b.add_virtual_target(), b.add_virtual_target()
    return b, x, y, b.is_equal(x, y)


def less_or_equal_circuit(pkg, max_allowed_value):
    """:159-179 assert_target_is_less_or_equal: one public input under the <= check, standard_recursion_config."""
    b = pkg.translate.CircuitBuilder(num_wires=135)
    t = b.add_virtual_target()
    b.register_public_input(t)
    pkg.translate.MemoryOperationsTranslator.add_restrictions_to_assert_target_is_less_or_equal_to(max_allowed_value, t, b)
    return b, t
