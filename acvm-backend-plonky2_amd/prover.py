"""ctypes binding of libp2gpu.so (include/p2gpu.h) with the reference's names.

Mirrors, for the hot path only:
  * ``CircuitData<F, C, D>``            -> :class:`CircuitData` (built from the circuit blob the
    Rust side exports once per circuit; see include/p2gpu.h)
  * ``circuit_data.prove(witnesses)``   -> :meth:`CircuitData.prove`
    (plonky2-backend/src/actions/prove_action.rs:96; test twin
    circuit_translation/tests/factories/utils.rs:26)
  * ``ProofWithPublicInputs::to_bytes`` -> :meth:`ProofWithPublicInputs.to_bytes`
    (prove_action.rs:75-78; compression stays on the Rust side)
Errors surface as :class:`P2GpuError` carrying the library's message, where the
reference would `unwrap()` an `anyhow::Error`.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

UINT64_MAX = (1 << 64) - 1


class P2GpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"p2gpu error {code}: {msg}")
        self.code = code


class _Timings(ctypes.Structure):
    _fields_ = [
        ("wires_commit_ms", ctypes.c_double),
        ("zs_commit_ms", ctypes.c_double),
        ("quotient_ms", ctypes.c_double),
        ("openings_ms", ctypes.c_double),
        ("fri_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
        ("h2d_ms", ctypes.c_double),
        ("pow_witness", ctypes.c_uint64),
    ]


class _WitnessReport(ctypes.Structure):
    """p2gpu_witness_report"""
    _fields_ = [
        ("gate_rows_failed", ctypes.c_uint64),
        ("copy_cells_failed", ctypes.c_uint64),
        ("noncanonical_cells", ctypes.c_uint64),
        ("gate_row", ctypes.c_uint32),
        ("gate_index", ctypes.c_uint32),
        ("gate_kind", ctypes.c_uint32),
        ("constraint", ctypes.c_uint32),
        ("constraint_value", ctypes.c_uint64),
        ("copy_cell", ctypes.c_uint32 * 2),
        ("copy_partner", ctypes.c_uint32 * 2),
        ("copy_values", ctypes.c_uint64 * 2),
        ("noncanonical_cell", ctypes.c_uint32 * 2),
    ]


class _VerifyReport(ctypes.Structure):
    """p2gpu_verify_report"""
    _fields_ = [("status", ctypes.c_int32), ("reason", ctypes.c_uint32), ("query", ctypes.c_uint32), ("index", ctypes.c_uint32)]


class VerifyReport:
    """The verdict on one proof of a batch (``p2gpu_verify_batch``).  `ok`; `reason`: the P2GPU_VR_* code of the check that
    failed (0: none); `query`, `index`: the query and the initial oracle or fold step the reason names, None where it names
    none (for a wrong length: the length given and the length the circuit fixes); `message`: the words of ``verify``'s error
    behind "proof rejected: " ("accepted" for a valid proof).  For a compressed proof (``p2gpu_verify_batch_compressed``) the
    reason may also be a P2GPU_VR_C_* code, a reject site of the decompression (16 and up): `message` is then the words of
    ``verify_compressed``'s error behind "malformed proof: "."""

    def __init__(self, raw, message):
        self.ok, self.reason, self.message = raw.status == 0, int(raw.reason), message
        self.query = None if raw.query == 0xFFFFFFFF else int(raw.query)
        self.index = None if raw.index == 0xFFFFFFFF else int(raw.index)

    def __eq__(self, other):
        return isinstance(other, VerifyReport) and (self.ok, self.reason, self.query, self.index, self.message) == \
            (other.ok, other.reason, other.query, other.index, other.message)

    def __repr__(self):
        return "VerifyReport(ok)" if self.ok else "VerifyReport(reason=%d, query=%r, index=%r, %r)" % (self.reason, self.query, self.index, self.message)


GATE_KIND_NAMES = ("NoopGate", "ConstantGate", "PublicInputGate", "ArithmeticGate", "BaseSumGate", "RandomAccessGate", "PoseidonGate",
                   "U32ArithmeticGate", "U32AddManyGate", "U32SubtractionGate", "U32RangeCheckGate", "ComparisonGate")


class WitnessReport:
    """What ``p2gpu_check_witness`` found in one wire matrix.  `first_gate`: (row, gate index, gate kind, constraint, value) of
    the lowest failing row and its lowest failing constraint; `first_copy`: ((row, col), (row, col) of sigma of it, the two
    values) of the flagged cell with the lowest key col << degree_bits | row; `first_noncanonical`: (row, col); each None where
    its count is 0.  With details: `row_status` [degree] uint16 (the first failing constraint of every row, 0xFFFF: none) and
    `cell_flags` [num_routed_wires][degree] uint8 (1: a flagged copy cell), else None.  `message`: the library's words for the
    first finding ("" for a clean report of a lone call)."""

    def __init__(self, raw, row_status=None, cell_flags=None, message=""):
        self.gate_rows_failed, self.copy_cells_failed = int(raw.gate_rows_failed), int(raw.copy_cells_failed)
        self.noncanonical_cells = int(raw.noncanonical_cells)
        self.first_gate = (int(raw.gate_row), int(raw.gate_index), int(raw.gate_kind), int(raw.constraint),
                           int(raw.constraint_value)) if self.gate_rows_failed else None
        self.first_copy = (tuple(int(x) for x in raw.copy_cell), tuple(int(x) for x in raw.copy_partner),
                           tuple(int(x) for x in raw.copy_values)) if self.copy_cells_failed else None
        self.first_noncanonical = tuple(int(x) for x in raw.noncanonical_cell) if self.noncanonical_cells else None
        self.row_status, self.cell_flags, self.message = row_status, cell_flags, message

    @property
    def ok(self):
        return not (self.gate_rows_failed or self.copy_cells_failed or self.noncanonical_cells)

    def __repr__(self):
        return "WitnessReport(ok)" if self.ok else "WitnessReport(gate_rows_failed=%d, copy_cells_failed=%d, noncanonical_cells=%d, first_gate=%r, " \
            "first_copy=%r, first_noncanonical=%r)" % (self.gate_rows_failed, self.copy_cells_failed, self.noncanonical_cells, self.first_gate,
                                                       self.first_copy, self.first_noncanonical)


_ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64)


class _DevBytes:
    """Zero-copy view of a device buffer for torch (``__cuda_array_interface__``)."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False),
                                         "version": 2}


def lib_path():
    # P2GPU_LIBRARY: an alternative build of the same library (A/B measurements of kernel variants only)
    return os.environ.get("P2GPU_LIBRARY") or os.path.join(_HERE, "libp2gpu.so")


def load_library():
    """Load libp2gpu.so.  Fails loudly when the HIP extension is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise P2GpuError(-8, f"{path} is missing: build it with __graft_entry__.build() (hipcc, gfx950)")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (same SONAME as
    # /opt/rocm's).  Importing torch FIRST makes libp2gpu.so bind to that already-loaded runtime,
    # so torch tensors (device memory, streams) and our kernels share one context; loading in
    # the other order maps two runtimes and the second one sees no devices.
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is part of the target image
        pass
    lib = ctypes.CDLL(path)
    vp, sz, u8p = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p
    lib.p2gpu_last_error.restype = ctypes.c_char_p
    lib.p2gpu_init.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    lib.p2gpu_circuit_create.argtypes = [u8p, sz, ctypes.POINTER(vp)]
    lib.p2gpu_circuit_destroy.argtypes = [vp]
    lib.p2gpu_circuit_destroy.restype = None
    lib.p2gpu_circuit_cap.argtypes = [vp, u8p]
    lib.p2gpu_circuit_digest.argtypes = [vp, u8p]
    lib.p2gpu_proof_size_bound.argtypes = [vp]
    lib.p2gpu_proof_size_bound.restype = sz
    lib.p2gpu_circuit_device.argtypes = [vp]
    lib.p2gpu_circuit_hash_bytes.argtypes = [vp]
    lib.p2gpu_prove.argtypes = [vp, vp, vp, ctypes.c_uint32, u8p, ctypes.POINTER(sz), ctypes.POINTER(_Timings)]
    lib.p2gpu_prove_dev.argtypes = lib.p2gpu_prove.argtypes
    lib.p2gpu_prove_routed.argtypes = lib.p2gpu_prove.argtypes
    a = lib.p2gpu_prove.argtypes
    lib.p2gpu_prove_sparse.argtypes = [a[0], a[1], ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32] + list(a[2:])
    lib.p2gpu_fill_witness.argtypes = [vp, vp]
    lib.p2gpu_witness_plan_create.argtypes = [vp, vp, sz, ctypes.POINTER(vp)]
    lib.p2gpu_witness_plan_build.argtypes = [vp, vp, sz, ctypes.POINTER(vp)]
    lib.p2gpu_witness_plan_export.argtypes = [vp, vp, vp, vp, vp]
    lib.p2gpu_witness_plan_create_gen.argtypes = [vp, vp, sz, vp, sz, ctypes.POINTER(vp)]
    lib.p2gpu_witness_plan_build_gen.argtypes = [vp, vp, sz, vp, sz, ctypes.POINTER(vp)]
    lib.p2gpu_witness_plan_export_generators.argtypes = [vp, vp, ctypes.POINTER(sz)]
    lib.p2gpu_witness_plan_create_genv.argtypes = [vp, vp, sz, vp, sz, vp, sz, ctypes.POINTER(vp)]
    lib.p2gpu_witness_plan_build_genv.argtypes = [vp, vp, sz, vp, sz, vp, sz, ctypes.POINTER(vp)]
    lib.p2gpu_witness_plan_export_generators_v.argtypes = [vp, vp, vp, vp]
    lib.p2gpu_witness_plan_destroy.argtypes = [vp]
    lib.p2gpu_witness_plan_destroy.restype = None
    lib.p2gpu_witness_plan_info.argtypes = [vp, vp, vp]
    lib.p2gpu_generate_witness.argtypes = [vp, vp, vp]
    lib.p2gpu_generate_witness_batch.argtypes = [vp, vp, sz, vp, vp, vp]
    lib.p2gpu_prove_seeds.argtypes = [vp, vp, vp, ctypes.c_uint32, u8p, ctypes.POINTER(sz), ctypes.POINTER(_Timings)]
    lib.p2gpu_prove_batch_dev.argtypes = [vp, vp, sz, vp, ctypes.c_uint32, u8p, vp]
    lib.p2gpu_prove_seeds_batch.argtypes = [vp, vp, sz, vp, ctypes.c_uint32, u8p, vp, vp]
    lib.p2gpu_prove_batch_max_degree_bits.restype = ctypes.c_uint32
    lib.p2gpu_prove_batch_info.argtypes = [vp, vp]
    lib.p2gpu_check_witness_dev.argtypes = [vp, vp, sz, vp, ctypes.c_uint32, vp, vp, vp]
    lib.p2gpu_check_witness.argtypes = [vp, vp, vp, ctypes.c_uint32, vp, vp, vp]
    lib.p2gpu_check_seeds.argtypes = [vp, vp, vp, ctypes.c_uint32, vp, vp, vp]
    lib.p2gpu_verify.argtypes = [vp, u8p, sz]
    lib.p2gpu_verify_batch.argtypes = [vp, u8p, vp, sz, vp]
    lib.p2gpu_verify_batch_host.argtypes = [vp, u8p, vp, sz, vp]
    lib.p2gpu_verify_reason.argtypes = [vp, ctypes.c_char_p, sz]
    lib.p2gpu_verify_batch_compressed.argtypes = [vp, u8p, vp, sz, vp]
    lib.p2gpu_verify_batch_compressed_host.argtypes = [vp, u8p, vp, sz, vp]
    lib.p2gpu_proof_decompress_batch.argtypes = [vp, u8p, vp, sz, vp, vp]
    lib.p2gpu_circuit_export_vk.argtypes = [vp, u8p, ctypes.POINTER(sz)]
    lib.p2gpu_circuit_export_vk_plonky2.argtypes = [vp, u8p, ctypes.POINTER(sz)]
    lib.p2gpu_verifier_create_plonky2.argtypes = [u8p, sz, ctypes.c_int, ctypes.POINTER(vp)]
    lib.p2gpu_verifier_create.argtypes = [u8p, sz, ctypes.POINTER(vp)]
    lib.p2gpu_proof_compress.argtypes = [vp, u8p, sz, u8p, ctypes.POINTER(sz)]
    lib.p2gpu_proof_decompress.argtypes = [vp, u8p, sz, u8p, ctypes.POINTER(sz)]
    lib.p2gpu_verify_compressed.argtypes = [vp, u8p, sz]
    lib.p2gpu_circuit_set.argtypes = [vp, ctypes.c_char_p, ctypes.c_uint64]
    lib.p2gpu_circuit_set_shard.argtypes = [vp, ctypes.c_int, ctypes.c_int, _ALLGATHER_FN, vp]
    lib.p2gpu_shard_unique_id.argtypes = [vp]
    lib.p2gpu_circuit_set_shard_rccl.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
    lib.p2gpu_kernel_stats.argtypes = [vp, ctypes.c_char_p, vp, vp, vp, ctypes.c_int]
    lib.p2gpu_ifft_batch.argtypes = [vp, sz, ctypes.c_uint, vp]
    lib.p2gpu_lde_batch.argtypes = [vp, sz, ctypes.c_uint, ctypes.c_uint, vp]
    lib.p2gpu_commit_values.argtypes = [vp, sz, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, u8p]
    lib.p2gpu_hash_rows.argtypes = [vp, sz, sz, u8p]
    lib.p2gpu_field_selftest.argtypes = [vp, vp, sz, vp]
    lib.p2gpu_field_selftest16.argtypes = [vp, vp, sz, vp]
    lib.p2gpu_forms_selftest.argtypes = [ctypes.c_uint, vp, sz, vp, vp]
    lib.p2gpu_plonk_stages.argtypes = [vp] * 11
    lib.p2gpu_device_info.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(sz)]
    lib.p2gpu_peer_access.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    lib.p2gpu_circuit_create_on.argtypes = [u8p, sz, ctypes.c_int, ctypes.POINTER(vp)]
    lib.p2gpu_circuit_build.argtypes = [vp, vp, ctypes.c_uint32, vp, vp, vp, sz, ctypes.c_uint32, ctypes.POINTER(vp)]
    lib.p2gpu_circuit_build_on.argtypes = [vp, vp, ctypes.c_uint32, vp, vp, vp, sz, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(vp)]
    lib.p2gpu_circuit_export_blob.argtypes = [vp, u8p, ctypes.POINTER(sz)]
    lib.p2gpu_peer_access.restype = ctypes.c_int
    lib.p2gpu_host_alloc.argtypes = [sz]
    lib.p2gpu_host_alloc.restype = vp
    lib.p2gpu_host_free.argtypes = [vp]
    lib.p2gpu_host_free.restype = None
    _LIB = lib
    return lib


def _check(rc):
    if rc != 0:
        raise P2GpuError(rc, load_library().p2gpu_last_error().decode(errors="replace"))


def _u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a


def init(devices=(0,)):
    """``p2gpu_init``: the HIP devices this process drives.  One id: one process per GPU.  Several ids: every
    ``CircuitData`` made afterwards is a device group and each ``prove`` is ONE proof coset-sharded over those GPUs from
    this single process (peer-to-peer exchanges between the ranks' streams, one host thread per rank inside the call) --
    the shape the reference's one ``circuit_data.prove`` call site (prove_action.rs:96) can drive.  The number of ids
    must divide the 8 LDE cosets; an id may repeat (ranks sharing a GPU: the functional test of this path on one GPU)."""
    lib = load_library()
    devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
    _check(lib.p2gpu_init(devs, len(devices)))


class _HostBlock:
    """Owner of one ``p2gpu_host_alloc`` block; the numpy view made over it keeps this object alive."""

    def __init__(self, nbytes):
        self._lib = load_library()
        self.ptr = self._lib.p2gpu_host_alloc(nbytes)
        if not self.ptr:
            raise P2GpuError(-3, self._lib.p2gpu_last_error().decode(errors="replace"))
        self.buf = (ctypes.c_uint8 * max(1, nbytes)).from_address(self.ptr)

    def __del__(self):
        if getattr(self, "ptr", None):
            self.buf = None
            self._lib.p2gpu_host_free(self.ptr)
            self.ptr = None


def host_array(shape, dtype=np.uint64):
    """A numpy array in page-locked host memory (``p2gpu_host_alloc``): a wire matrix built in place here uploads by
    direct DMA inside ``prove`` instead of being staged by the HIP runtime on the calling thread."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    blk = _HostBlock(nbytes)
    arr = np.frombuffer(blk.buf, dtype=dtype, count=nbytes // np.dtype(dtype).itemsize).reshape(shape)
    _HOST_BLOCKS[id(blk)] = blk  # freed by host_free(arr) or at interpreter exit; a view may outlive `arr` itself
    arr.flags.writeable = True
    return arr


_HOST_BLOCKS = {}


def host_free(arr):
    """Release the block behind an array returned by ``host_array`` (the array must not be used afterwards)."""
    addr = arr.ctypes.data
    for k, blk in list(_HOST_BLOCKS.items()):
        if blk.ptr == addr:
            del _HOST_BLOCKS[k]
            blk.__del__()
            return
    raise P2GpuError(-1, "host_free: not an array from host_array")


def device_info():
    lib = load_library()
    name = ctypes.create_string_buffer(256)
    cu = ctypes.c_int()
    mem = ctypes.c_size_t()
    _check(lib.p2gpu_device_info(name, 256, ctypes.byref(cu), ctypes.byref(mem)))
    return {"name": name.value.decode(), "cu_count": cu.value, "hbm_bytes": mem.value}


def peer_access():
    """n x n matrix for the device ids of the last ``init``: 1 = device a reaches device b's memory directly (peer copies
    over xGMI), 0 = it does not (staged through the host), -1 = the same device (``p2gpu_peer_access``)."""
    lib = load_library()
    n = lib.p2gpu_peer_access(None, 0)
    if n < 0:
        _check(n)
    m = (ctypes.c_int * (n * n))()
    _check(min(0, lib.p2gpu_peer_access(m, n * n)))
    return [[int(m[a * n + b]) for b in range(n)] for a in range(n)]


class ProofWithPublicInputs:
    """Uncompressed proof bytes in plonky2's ``ProofWithPublicInputs::to_bytes`` layout."""

    def __init__(self, data, timings=None):
        self._data = bytes(data)
        self.timings = timings or {}

    def to_bytes(self):
        return self._data

    def __len__(self):
        return len(self._data)

    def __eq__(self, other):
        return isinstance(other, ProofWithPublicInputs) and self._data == other._data


class CircuitData:
    """Prover-side circuit handle (device-resident constants/sigmas oracle, root tables)."""

    def __init__(self, blob, device=None):
        """device: None = what ``init`` selected (several ids: a device group, every proof sharded over them); an id of that
        list = a plain handle on that one device (``p2gpu_circuit_create_on``: replicas across GPUs from one process)."""
        lib = load_library()
        self._lib = lib
        self._blob = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob)
        hdr = self._blob[:256].view(np.uint32)
        self.degree_bits = int(hdr[2])
        self.num_wires = int(hdr[3])
        self.num_routed_wires = int(hdr[4])
        self.rate_bits = int(hdr[9])
        self.cap_height = int(hdr[10])
        self.num_public_inputs = int(hdr[24])
        self._h = ctypes.c_void_p()
        if device is None:
            _check(lib.p2gpu_circuit_create(self._blob.ctypes.data, self._blob.nbytes, ctypes.byref(self._h)))
        else:
            _check(lib.p2gpu_circuit_create_on(self._blob.ctypes.data, self._blob.nbytes, int(device), ctypes.byref(self._h)))
        self._bound = lib.p2gpu_proof_size_bound(self._h)

    @classmethod
    def from_blob(cls, blob):
        return cls(blob)

    @classmethod
    def build(cls, degree_bits, gates, row_gate, row_constants, copies, num_public_inputs=0, num_wires=234, num_routed_wires=80,
              num_challenges=2, quotient_degree_factor=8, rate_bits=3, cap_height=4, proof_of_work_bits=16, num_query_rounds=28,
              hasher=0, device=None):
        """``builder.build::<C>()`` on the device (``p2gpu_circuit_build``): the arguments of ``build_blob`` plus the hasher
        (0 KeccakHash<25>, 1 PoseidonHash), straight to a prover handle -- selector columns, row -> gate and the sigma
        polynomials are made by kernels from the uploaded gate rows and copy pairs, no blob passes through host memory.
        The handle is the one ``CircuitData(build_blob(...))`` gives; ``to_blob()`` reads the blob back to cache it.
        device: as for the constructor."""
        lib = load_library()
        bp, gd, rg, rc, cp = _build_args(degree_bits, gates, row_gate, row_constants, copies, num_public_inputs, num_wires, num_routed_wires,
                                         num_challenges, quotient_degree_factor, rate_bits, cap_height, proof_of_work_bits, num_query_rounds)
        self = cls.__new__(cls)
        self._lib = lib
        self._blob = None
        self.degree_bits, self.num_wires, self.num_routed_wires = int(degree_bits), int(num_wires), int(num_routed_wires)
        self.rate_bits, self.cap_height, self.num_public_inputs = int(rate_bits), int(cap_height), int(num_public_inputs)
        self._h = ctypes.c_void_p()
        args = [ctypes.byref(bp), gd, len(gates), rg.ctypes.data, rc.ctypes.data if rc.size else None, cp.ctypes.data if cp.size else None,
                len(cp), int(hasher)]
        if device is None:
            _check(lib.p2gpu_circuit_build(*args, ctypes.byref(self._h)))
        else:
            _check(lib.p2gpu_circuit_build_on(*args, int(device), ctypes.byref(self._h)))
        self._bound = lib.p2gpu_proof_size_bound(self._h)
        return self

    def to_blob(self):
        """The circuit blob of this handle, read back from the device (``p2gpu_circuit_export_blob``): for a handle from
        ``build`` exactly what ``build_blob`` returns for the same arguments, with the hasher in header word 22."""
        ln = ctypes.c_size_t(0)
        _check(self._lib.p2gpu_circuit_export_blob(self._h, None, ctypes.byref(ln)))
        out = np.zeros(ln.value, dtype=np.uint8)
        _check(self._lib.p2gpu_circuit_export_blob(self._h, out.ctypes.data, ctypes.byref(ln)))
        return out[:ln.value]

    @property
    def degree(self):
        return 1 << self.degree_bits

    def constants_sigmas_cap(self):
        out = np.zeros(self.hash_bytes() << self.cap_height, dtype=np.uint8)
        _check(self._lib.p2gpu_circuit_cap(self._h, out.ctypes.data))
        return out.tobytes()

    def circuit_digest(self):
        out = np.zeros(self.hash_bytes(), dtype=np.uint8)
        _check(self._lib.p2gpu_circuit_digest(self._h, out.ctypes.data))
        return out.tobytes()

    def hash_bytes(self):
        """Digest size of the circuit's hasher: 25 (KeccakHash<25>) or 32 (PoseidonHash)."""
        return int(self._lib.p2gpu_circuit_hash_bytes(self._h))

    def device_index(self):
        """HIP device the handle's buffers and streams live on."""
        return int(self._lib.p2gpu_circuit_device(self._h))

    def set(self, key, value):
        _check(self._lib.p2gpu_circuit_set(self._h, key.encode(), ctypes.c_uint64(value)))

    def set_shard(self, rank, world, group=None, transport=None):
        """Coset-shard every following proof over the `world` ranks of `group` (one process per GPU;
        torch.distributed must be initialised when world > 1).

        transport "rccl" (default whenever the process group's backend is nccl): the library itself
        calls RCCL (ncclAllGather on its own HIP stream, xGMI on a real node) -- torch.distributed is used
        once, to broadcast the 128-byte ncclUniqueId.  transport "callback" (default for gloo, i.e. the
        CPU-side tests): the library hands device buffers to a host callback that gathers them with
        torch.distributed, staging through host tensors."""
        import torch
        import torch.distributed as dist

        backend = dist.get_backend(group) if (world > 1 or (dist.is_available() and dist.is_initialized())) else None
        if transport is None:
            transport = "rccl" if backend == "nccl" else "callback"
        if transport == "rccl":
            idbuf = np.zeros(128, dtype=np.uint8)
            if rank == 0:
                _check(self._lib.p2gpu_shard_unique_id(idbuf.ctypes.data))
            if world > 1:
                if backend == "nccl":
                    t = torch.from_numpy(idbuf).cuda()
                    dist.broadcast(t, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
                    idbuf = t.cpu().numpy()
                else:
                    t = torch.from_numpy(idbuf)
                    dist.broadcast(t, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
                    idbuf = t.numpy()
            idbuf = np.ascontiguousarray(idbuf)
            _check(self._lib.p2gpu_circuit_set_shard_rccl(self._h, rank, world, idbuf.ctypes.data))
            self._shard_cb = None
            self.shard = (rank, world)
            return
        if world > 1:

            def _allgather(_ctx, send, recv, nbytes):
                try:
                    s = torch.as_tensor(_DevBytes(send, nbytes), device="cuda")
                    r = torch.as_tensor(_DevBytes(recv, nbytes * world), device="cuda")
                    if backend == "nccl":
                        dist.all_gather_into_tensor(r, s, group=group)
                    else:
                        out = torch.empty(nbytes * world, dtype=torch.uint8)
                        dist.all_gather_into_tensor(out, s.cpu(), group=group)
                        r.copy_(out)
                    torch.cuda.synchronize()
                    return 0
                except Exception as e:  # never let an exception cross the C ABI
                    self._shard_error = e
                    return -1

            self._shard_cb = _ALLGATHER_FN(_allgather)  # keep alive as long as the handle
        else:
            self._shard_cb = _ALLGATHER_FN(0)
        _check(self._lib.p2gpu_circuit_set_shard(self._h, rank, world, self._shard_cb, None))
        self.shard = (rank, world)

    def kernel_stats(self):
        cap = 64
        names = ctypes.create_string_buffer(64 * cap)
        ms = np.zeros(cap, dtype=np.float64)
        by = np.zeros(cap, dtype=np.float64)
        ln = np.zeros(cap, dtype=np.uint64)
        k = self._lib.p2gpu_kernel_stats(self._h, names, ms.ctypes.data, by.ctypes.data, ln.ctypes.data, cap)
        out = {}
        for i in range(max(k, 0)):
            nm = names.raw[64 * i:64 * (i + 1)].split(b"\0", 1)[0].decode()
            out[nm] = {"ms": float(ms[i]), "bytes": float(by[i]), "launches": int(ln[i])}
        return out

    def prove(self, wires, public_inputs=()):
        """``circuit_data.prove(witnesses)``: `wires` is the full witness matrix
        [num_wires][degree] (numpy uint64 on the host, or a torch tensor on the
        circuit's GPU, which is read in place)."""
        pis = _u64(np.array(list(public_inputs), dtype=np.uint64))
        out = np.zeros(self._bound, dtype=np.uint8)
        plen = ctypes.c_size_t(out.nbytes)
        tm = _Timings()
        expect = self.num_wires * self.degree
        if hasattr(wires, "data_ptr") and getattr(wires, "is_cuda", False):
            if wires.numel() != expect or wires.element_size() != 8 or not wires.is_contiguous():
                raise P2GpuError(-7, "wires tensor must be contiguous int64/uint64 [num_wires][degree]")
            if wires.device.index != self.device_index():
                raise P2GpuError(-7, f"wires tensor lives on cuda:{wires.device.index}, the circuit on cuda:{self.device_index()}")
            rc = self._lib.p2gpu_prove_dev(self._h, ctypes.c_void_p(wires.data_ptr()), pis.ctypes.data, len(pis),
                                           out.ctypes.data, ctypes.byref(plen), ctypes.byref(tm))
        else:
            w = _u64(wires)
            if w.size != expect:
                raise P2GpuError(-7, f"wires must be [num_wires={self.num_wires}][degree={self.degree}]")
            rc = self._lib.p2gpu_prove(self._h, w.ctypes.data, pis.ctypes.data, len(pis), out.ctypes.data,
                                       ctypes.byref(plen), ctypes.byref(tm))
        _check(rc)
        t = {f: getattr(tm, f) for f, _ in _Timings._fields_}
        return ProofWithPublicInputs(out[:plen.value].tobytes(), t)

    # the words of the lone call for the codes a member of a batch can end with
    _MEMBER_WORDS = {-5: "witness does not satisfy the circuit: the plonk identity fails at zeta (vanishing != Z_H * quotient)",
                     -4: "Opening point is in the subgroup."}

    def _batch_pis(self, batch, public_inputs):
        pis = [()] * batch if public_inputs is None else [list(p) for p in public_inputs]
        if len(pis) != batch:
            raise P2GpuError(-7, f"{batch} lists of public inputs expected, {len(pis)} given")
        n_pi = len(pis[0])
        if any(len(p) != n_pi for p in pis):
            raise P2GpuError(-7, "every member needs the same number of public inputs")
        return _u64(np.array(pis, dtype=np.uint64).reshape(batch, n_pi)), n_pi

    def _batch_results(self, rc, out, status):
        """Per member the proof or the error the lone call raises; a code that belongs to no member raises here."""
        if rc not in (0, -4, -5) or (rc and not any(int(s) == rc for s in status)):
            _check(rc)
        res = []
        for b, st in enumerate(status):
            st = int(st)
            res.append(ProofWithPublicInputs(out[b].tobytes()) if st == 0 else P2GpuError(st, self._MEMBER_WORDS.get(st, "error %d" % st)))
        return res

    def prove_batch(self, wires, public_inputs=None):
        """``p2gpu_prove_batch_dev``: the proofs of B witnesses of this (small) circuit in one call.  `wires`: an int64 tensor
        [B][num_wires][degree] on the circuit's GPU (the layout of ``WitnessPlan.generate_batch``), only read;
        `public_inputs`: one list per member.  Returns per member the ``ProofWithPublicInputs`` -- the bytes ``prove`` gives for
        that matrix -- or the ``P2GpuError`` the lone call raises."""
        import torch

        if not (hasattr(wires, "data_ptr") and getattr(wires, "is_cuda", False)) or wires.dim() != 3 or not wires.is_contiguous() \
                or wires.element_size() != 8 or wires[0].numel() != self.num_wires * self.degree:
            raise P2GpuError(-7, "wires tensor must be contiguous int64/uint64 [batch][num_wires][degree] on the GPU")
        if wires.device.index != self.device_index():
            raise P2GpuError(-7, f"wires tensor lives on cuda:{wires.device.index}, the circuit on cuda:{self.device_index()}")
        batch = wires.shape[0]
        pis, n_pi = self._batch_pis(batch, public_inputs)
        out = np.zeros((batch, self._bound), dtype=np.uint8)
        status = np.zeros(batch, dtype=np.intc)
        torch.cuda.current_stream(wires.device).synchronize()
        rc = self._lib.p2gpu_prove_batch_dev(self._h, ctypes.c_void_p(wires.data_ptr()), batch, pis.ctypes.data, n_pi, out.ctypes.data,
                                             status.ctypes.data)
        return self._batch_results(rc, out, status)

    def prove_batch_info(self):
        """``p2gpu_prove_batch_info``: launches of the last slab, proofs in it, bytes of the slab buffers, the byte budget."""
        v = np.zeros(4, dtype=np.uint64)
        _check(self._lib.p2gpu_prove_batch_info(self._h, v.ctypes.data))
        return {"launches": int(v[0]), "slab": int(v[1]), "arena_bytes": int(v[2]), "budget_bytes": int(v[3])}

    def plonk_stages(self, wires, pi_hash, betas, gammas, alphas, zp_in=None):
        """Prover phases 1-3 on caller-chosen challenges (``p2gpu_plonk_stages``, a test bed: no proof calls it).  Returns a
        dict: ``zp`` [K (1 + PP)][n] as phase 2 computed it (before ``zp_in`` replaces it), ``qvals`` [K][2^rate_bits][n],
        ``quot`` [K 2^rate_bits][n] (natural-order coefficients), ``caps`` (wires, zs, quotient) as bytes."""
        hdr = (self._blob if self._blob is not None else self.to_blob())[:256].view(np.uint32)
        K, PP, C, n = int(hdr[7]), int(hdr[26]), 1 << self.rate_bits, self.degree
        w = _u64(wires)
        if w.size != self.num_wires * n:
            raise P2GpuError(-7, f"wires must be [num_wires={self.num_wires}][degree={n}]")
        ch = [_u64(np.array([int(x) for x in v], dtype=np.uint64)) for v in (pi_hash, betas, gammas, alphas)]
        if ch[0].size != 4 or any(v.size != K for v in ch[1:]):
            raise P2GpuError(-7, f"pi_hash must hold 4 words, betas / gammas / alphas {K} each")
        zi = None
        if zp_in is not None:
            zi = _u64(zp_in)
            if zi.size != K * (1 + PP) * n:
                raise P2GpuError(-7, f"zp_in must be [{K * (1 + PP)}][{n}]")
        zp = np.zeros((K * (1 + PP), n), dtype=np.uint64)
        qv = np.zeros((K, C, n), dtype=np.uint64)
        quot = np.zeros((K * C, n), dtype=np.uint64)
        hb = self.hash_bytes() << self.cap_height
        caps = np.zeros(3 * hb, dtype=np.uint8)
        _check(self._lib.p2gpu_plonk_stages(self._h, w.ctypes.data, ch[0].ctypes.data, ch[1].ctypes.data, ch[2].ctypes.data, ch[3].ctypes.data,
                                            zi.ctypes.data if zi is not None else None, zp.ctypes.data, qv.ctypes.data, quot.ctypes.data,
                                            caps.ctypes.data))
        cb = caps.tobytes()
        return {"zp": zp, "qvals": qv, "quot": quot, "caps": (cb[:hb], cb[hb:2 * hb], cb[2 * hb:])}

    def _check_call(self, call, batch, public_inputs, details):
        """Run call(pis pointer, n_pi, reports pointer, row_status pointer, cell_flags pointer) -> rc of one of the check entry
        points over `batch` witnesses; [WitnessReport].  A report that is not clean does not raise: -5 is the answer asked for."""
        rows = [[int(v) for v in p] for p in public_inputs]
        if len({len(r) for r in rows}) != 1:
            raise P2GpuError(-7, "every witness takes the same number of public inputs")
        pis = _u64(np.array(rows, dtype=np.uint64).reshape(batch, len(rows[0])))
        reports = (_WitnessReport * batch)()
        status = np.zeros((batch, self.degree), dtype=np.uint16) if details else None
        flags = np.zeros((batch, self.num_routed_wires, self.degree), dtype=np.uint8) if details else None
        rc = call(pis.ctypes.data if pis.size else None, pis.shape[1], reports, status.ctypes.data if details else None,
                  flags.ctypes.data if details else None)
        # (-5 with every count zero is no report: the level walk in front of p2gpu_check_seeds refused the values)
        if rc != -5 or not any(r.gate_rows_failed or r.copy_cells_failed or r.noncanonical_cells for r in reports):
            _check(rc)
        msg = self._lib.p2gpu_last_error().decode(errors="replace") if rc else ""
        return [WitnessReport(reports[b], status[b] if details else None, flags[b] if details else None, msg) for b in range(batch)]

    def check_witness(self, wires, public_inputs=(), details=False):
        """``p2gpu_check_witness`` / ``_dev``: which gate rows and copy constraints the witness matrix [num_wires][degree] breaks
        and which of its words are no canonical field elements, found on the GPU; a :class:`WitnessReport`.  `wires` as
        :meth:`prove` takes it: numpy uint64 on the host, a torch tensor on the circuit's GPU or any object with a
        ``__cuda_array_interface__`` there (read in place).  ``details=True`` also brings back the per-row and per-cell results."""
        expect = self.num_wires * self.degree
        ptr = None
        if hasattr(wires, "data_ptr") and getattr(wires, "is_cuda", False):
            import torch

            if wires.numel() != expect or wires.element_size() != 8 or not wires.is_contiguous():
                raise P2GpuError(-7, "wires tensor must be contiguous int64/uint64 [num_wires][degree]")
            if wires.device.index != self.device_index():
                raise P2GpuError(-7, f"wires tensor lives on cuda:{wires.device.index}, the circuit on cuda:{self.device_index()}")
            torch.cuda.current_stream(wires.device).synchronize()   # (the library reads on the handle's own stream)
            ptr = wires.data_ptr()
        elif hasattr(wires, "__cuda_array_interface__"):
            cai = wires.__cuda_array_interface__
            if int(np.prod(cai["shape"])) * np.dtype(cai["typestr"]).itemsize != 8 * expect:
                raise P2GpuError(-7, f"the device buffer must hold [num_wires={self.num_wires}][degree={self.degree}] 64-bit words")
            ptr = cai["data"][0]
        if ptr is not None:
            return self._check_call(lambda pis, n_pi, rep, st, fl: self._lib.p2gpu_check_witness_dev(
                self._h, ctypes.c_void_p(ptr), 1, pis, n_pi, rep, st, fl), 1, [public_inputs], details)[0]
        w = _u64(wires)
        if w.size != expect:
            raise P2GpuError(-7, f"wires must be [num_wires={self.num_wires}][degree={self.degree}]")
        return self._check_call(lambda pis, n_pi, rep, st, fl: self._lib.p2gpu_check_witness(
            self._h, w.ctypes.data, pis, n_pi, rep, st, fl), 1, [public_inputs], details)[0]

    def check_witness_batch(self, wires_dev, public_inputs=None, details=False):
        """The same for a torch tensor [batch][num_wires][degree] on the circuit's GPU (the layout of
        ``WitnessPlan.generate_batch``), `public_inputs` one list per witness; [WitnessReport]."""
        import torch

        if not (hasattr(wires_dev, "data_ptr") and getattr(wires_dev, "is_cuda", False)) or wires_dev.dim() != 3 or not wires_dev.is_contiguous() \
                or wires_dev.element_size() != 8 or wires_dev[0].numel() != self.num_wires * self.degree:
            raise P2GpuError(-7, "wires tensor must be contiguous int64/uint64 [batch][num_wires][degree] on the GPU")
        if wires_dev.device.index != self.device_index():
            raise P2GpuError(-7, f"wires tensor lives on cuda:{wires_dev.device.index}, the circuit on cuda:{self.device_index()}")
        batch = wires_dev.shape[0]
        pis = [()] * batch if public_inputs is None else list(public_inputs)
        if len(pis) != batch:
            raise P2GpuError(-7, f"{batch} lists of public inputs expected, {len(pis)} given")
        torch.cuda.current_stream(wires_dev.device).synchronize()
        return self._check_call(lambda p, n_pi, rep, st, fl: self._lib.p2gpu_check_witness_dev(
            self._h, ctypes.c_void_p(wires_dev.data_ptr()), batch, p, n_pi, rep, st, fl), batch, pis, details)

    def fill_witness(self, wires_dev):
        """Run the gates' row-local generators on a device wire matrix (torch tensor, in place)."""
        if not (hasattr(wires_dev, "data_ptr") and getattr(wires_dev, "is_cuda", False)):
            raise P2GpuError(-7, "fill_witness needs a torch tensor on the GPU")
        if wires_dev.numel() != self.num_wires * self.degree or not wires_dev.is_contiguous():
            raise P2GpuError(-7, "wires tensor must be contiguous [num_wires][degree]")
        _check(self._lib.p2gpu_fill_witness(self._h, ctypes.c_void_p(wires_dev.data_ptr())))
        return wires_dev

    def witness_plan(self, seed_cells, compile="host", generators=None):
        """``p2gpu_witness_plan_create``: the plan that turns the values of `seed_cells` ([(row, col)]: the cells the
        caller assigns per proof, ``pw.set_target`` on the Rust side) into the whole witness on the GPU.
        ``compile="device"``: the same plan through ``p2gpu_witness_plan_build``, compiled on the GPU.
        ``generators``: the generators that are no gate's own, [("equality", (cell_x, cell_y, cell_equal, cell_inv))] with
        (row, col) cells, and ("biguint_divrem", (a_cells, b_cells, div_cells, rem_cells)) with the limbs' cells, least
        significant first, and ("nonnative_add" | "nonnative_sub" | "nonnative_mul" | "nonnative_inv", (a_cells, b_cells, first
        target's cells, second target's cells), "secp256k1_base" | "secp256k1_scalar") for the four nonnative generators, and
        ("glv_decompose", (k_cells, (), the cells of k1's then k2's limbs, (k1_neg cell, k2_neg cell))) for the GLV decomposition
        (``translate.CircuitBuilder.generators()``); the plan then comes from
        ``p2gpu_witness_plan_create_gen`` / ``_build_gen``, or from ``_create_genv`` / ``_build_genv`` when a generator has
        another number of cells than four or names a field."""
        return WitnessPlan(self, seed_cells, compile=compile, generators=generators)

    def prove_routed(self, routed, public_inputs=()):
        """Prove from the routed columns only ([num_routed_wires][degree], host): gate-internal
        columns are derived on the GPU by the row-local generators."""
        pis = _u64(np.array(list(public_inputs), dtype=np.uint64))
        r = _u64(routed)
        if r.size != self.num_routed_wires * self.degree:
            raise P2GpuError(-7, f"routed must be [num_routed_wires={self.num_routed_wires}][degree={self.degree}]")
        out = np.zeros(self._bound, dtype=np.uint8)
        plen = ctypes.c_size_t(out.nbytes)
        tm = _Timings()
        _check(self._lib.p2gpu_prove_routed(self._h, r.ctypes.data, pis.ctypes.data, len(pis), out.ctypes.data,
                                            ctypes.byref(plen), ctypes.byref(tm)))
        return ProofWithPublicInputs(out[:plen.value].tobytes(), {f: getattr(tm, f) for f, _ in _Timings._fields_})

    def prove_sparse(self, wires, ncols, row, public_inputs=(), tail=None):
        """Prove from the first `ncols` wire columns plus ONE value for each of the others (``p2gpu_prove_sparse``):
        column j >= ncols is zero in every row but `row`, where it holds ``tail[j - ncols]`` -- what plonky2 leaves
        in the wires no gate of a circuit uses.  `wires` is the full [num_wires][degree] matrix (the tail is then
        read off row `row`) or just its first `ncols` columns with `tail` given.  Same bytes as ``prove``; only
        `ncols` columns cross PCIe."""
        pis = _u64(np.array(list(public_inputs), dtype=np.uint64))
        W, n = self.num_wires, self.degree
        w = _u64(wires)
        if not (0 <= ncols <= W and 0 <= row < n):
            raise P2GpuError(-7, f"prove_sparse: ncols {ncols} of {W} wires, row {row} of {n}")
        if tail is None:
            if w.size != W * n:
                raise P2GpuError(-7, f"wires must be [num_wires={W}][degree={n}] when no tail is given")
            full = w.reshape(W, n)
            tail = np.ascontiguousarray(full[ncols:, row])
            w = np.ascontiguousarray(full[:ncols]).reshape(-1)
        else:
            tail = _u64(np.asarray(tail, dtype=np.uint64))
        if ncols > W or w.size != ncols * n or tail.size != W - ncols:
            raise P2GpuError(-7, f"prove_sparse: [{ncols}][{n}] dense columns and {W - ncols} tail values expected")
        out = np.zeros(self._bound, dtype=np.uint8)
        plen = ctypes.c_size_t(out.nbytes)
        tm = _Timings()
        _check(self._lib.p2gpu_prove_sparse(self._h, w.ctypes.data if w.size else None, ncols,
                                            tail.ctypes.data if tail.size else None, row,
                                            pis.ctypes.data, len(pis), out.ctypes.data, ctypes.byref(plen), ctypes.byref(tm)))
        return ProofWithPublicInputs(out[:plen.value].tobytes(), {f: getattr(tm, f) for f, _ in _Timings._fields_})

    def verify(self, proof):
        """``circuit_data.verify(proof)``: raises P2GpuError(P2GPU_E_VERIFY) when the proof is
        rejected (the failed check is the message), returns None when it is accepted."""
        _verify(self._lib, self._h, proof)

    def verify_batch(self, proofs):
        """``p2gpu_verify_batch`` on this handle's device and stream: one :class:`VerifyReport` per proof.  An invalid proof
        raises nothing; P2GpuError is for argument and device errors."""
        return _verify_batch(self._lib, self._h, proofs, True)

    def verify_batch_compressed(self, proofs):
        """``p2gpu_verify_batch_compressed`` on this handle's device and stream: ``verify_batch`` for compressed proofs (the
        on-disk format), decompressed on the device; the verdict of each is ``verify_compressed``'s."""
        return _verify_batch(self._lib, self._h, proofs, True, compressed=True)

    def decompress_batch(self, proofs):
        """``p2gpu_proof_decompress_batch``: the device's decompression of each compressed proof, read back -- per member a
        :class:`ProofWithPublicInputs` with the bytes of ``decompress``, or the :class:`P2GpuError` ``decompress`` raises."""
        return _decompress_batch(self._lib, self._h, proofs)

    def verifier_data(self):
        """``circuit_data.verifier_data()``: the verifier's share of the circuit."""
        return VerifierCircuitData(self.verifier_blob())

    def verifier_blob(self):
        """Bytes of the verifier's share (header, gate table, constants_sigmas cap, digest, k_is)."""
        n = ctypes.c_size_t(0)
        _check(self._lib.p2gpu_circuit_export_vk(self._h, None, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        _check(self._lib.p2gpu_circuit_export_vk(self._h, out.ctypes.data, ctypes.byref(n)))
        return out[:n.value].tobytes()

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.p2gpu_circuit_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WitnessPlan:
    """Witness generation on the GPU for one circuit and one set of seed cells (``p2gpu_witness_plan``).  Close it before
    the circuit."""

    GENERATOR_KINDS = {"equality": 0, "biguint_divrem": 1}   # p2gpu.h P2GPU_GEN_EQUALITY, P2GPU_GEN_BIGUINT_DIVREM
    # the nonnative generators, given as (kind, groups, field): p2gpu.h P2GPU_GEN_NONNATIVE_*, P2GPU_FIELD_*; the record's kind
    # word is kind | field << 8
    NONNATIVE_KINDS = {"nonnative_add": 2, "nonnative_sub": 3, "nonnative_mul": 4, "nonnative_inv": 5}
    NONNATIVE_FIELDS = {"secp256k1_base": 0, "secp256k1_scalar": 1}
    # the GLV decomposition, given as (kind, groups) like the first two: p2gpu.h P2GPU_GEN_GLV_DECOMPOSE (6 and 7 are reserved).
    # A table of its own: GENERATOR_KINDS is stated as exactly those two kinds by the tests of the _genv ABI
    GLV_KINDS = {"glv_decompose": 8}

    @classmethod
    def _kind_word(cls, gen):
        """The kind word of a generator (kind, cells) or (kind, cells, field); a kind or a field may be given by its number."""
        kind = gen[0]
        if isinstance(kind, str):
            kind = cls.GENERATOR_KINDS[kind] if kind in cls.GENERATOR_KINDS else cls.NONNATIVE_KINDS.get(kind, cls.GLV_KINDS.get(kind, kind))
        if len(gen) > 2:
            field = cls.NONNATIVE_FIELDS.get(gen[2], gen[2]) if isinstance(gen[2], str) else gen[2]
            if isinstance(kind, str) or isinstance(field, str):
                raise P2GpuError(-7, f"unknown generator kind or field in {gen[0]!r}, {gen[2]!r}")
            return int(kind) | int(field) << 8
        if isinstance(kind, str):
            raise P2GpuError(-7, f"unknown generator kind {kind!r}")
        return kind

    def __init__(self, circuit, seed_cells, compile="host", generators=None):
        if compile not in ("host", "device"):
            raise P2GpuError(-7, f'compile must be "host" or "device", not {compile!r}')
        self._cd, self._lib = circuit, circuit._lib
        cells = np.ascontiguousarray(np.array(list(seed_cells), dtype=np.int64).reshape(-1, 2))
        if cells.size and (cells.min() < 0 or cells.max() >= 1 << 32):
            raise P2GpuError(-7, "seed cells are (row, col) pairs of unsigned 32-bit numbers")
        cells = cells.astype(np.uint32)
        self.num_seeds = len(cells)
        self._h = ctypes.c_void_p()
        if generators is None:
            make = self._lib.p2gpu_witness_plan_build if compile == "device" else self._lib.p2gpu_witness_plan_create
            _check(make(circuit._h, cells.ctypes.data if cells.size else None, len(cells), ctypes.byref(self._h)))
            return
        generators = list(generators)
        if any(len(g) > 2 or self._groups(g[1]) is not None for g in generators):
            self._init_genv(circuit, cells, compile, generators)
            return
        # p2gpu_generator records: kind, then four (row, col) pairs; a kind may be given by its number
        recs = np.zeros((len(generators), 9), dtype=np.int64)
        for i, (kind, gcells) in enumerate(generators):
            recs[i, 0] = self._kind_word((kind, gcells))
            recs[i, 1:] = np.array(list(gcells), dtype=np.int64).reshape(8)
        if recs.size and (recs.min() < 0 or recs.max() >= 1 << 32):
            raise P2GpuError(-7, "a generator is a kind and four (row, col) cells of unsigned 32-bit numbers")
        recs = np.ascontiguousarray(recs.astype(np.uint32))
        make = self._lib.p2gpu_witness_plan_build_gen if compile == "device" else self._lib.p2gpu_witness_plan_create_gen
        _check(make(circuit._h, cells.ctypes.data if cells.size else None, len(cells), recs.ctypes.data if recs.size else None, len(recs),
                    ctypes.byref(self._h)))

    @staticmethod
    def _groups(gcells):
        """The four cell groups of a generator given as (a_cells, b_cells, div_cells, rem_cells), None for four plain cells."""
        gcells = list(gcells)
        if len(gcells) == 4 and all(len(g) == 2 and all(isinstance(v, (int, np.integer)) for v in g) for g in gcells):
            return None
        return [[tuple(cell) for cell in grp] for grp in gcells]

    def _init_genv(self, circuit, cells, compile, generators):
        """p2gpu_generator_v records (kind, shape[4]) and the flat (row, col) list of their cells: the entry points for
        generators with any number of cells."""
        recs, flat = np.zeros((len(generators), 5), dtype=np.int64), []
        for i, gen in enumerate(generators):
            gcells = gen[1]
            groups = self._groups(gcells) or [[tuple(cell)] for cell in gcells]
            if len(groups) != 4:
                raise P2GpuError(-7, "a generator is a kind and four groups of (row, col) cells")
            recs[i, 0] = self._kind_word(gen)
            recs[i, 1:] = [len(g) for g in groups]
            flat += [cell for g in groups for cell in g]
        flat = np.array(flat, dtype=np.int64).reshape(-1, 2)
        if (recs.size and (recs.min() < 0 or recs.max() >= 1 << 32)) or (flat.size and (flat.min() < 0 or flat.max() >= 1 << 32)):
            raise P2GpuError(-7, "a generator is a kind, a shape and (row, col) cells of unsigned 32-bit numbers")
        recs, flat = np.ascontiguousarray(recs.astype(np.uint32)), np.ascontiguousarray(flat.astype(np.uint32))
        make = self._lib.p2gpu_witness_plan_build_genv if compile == "device" else self._lib.p2gpu_witness_plan_create_genv
        _check(make(circuit._h, cells.ctypes.data if cells.size else None, len(cells), recs.ctypes.data if recs.size else None, len(recs),
                    flat.ctypes.data if flat.size else None, len(flat), ctypes.byref(self._h)))

    def _values(self, values):
        v = _u64(np.array([int(x) for x in values], dtype=np.uint64))
        if v.size != self.num_seeds:
            raise P2GpuError(-7, f"{self.num_seeds} seed values expected, {v.size} given")
        return v

    def info(self):
        """Shape of the schedule, the host time of the plan's compilation and the device time of the last level walk."""
        counts, ms = np.zeros(5, dtype=np.uint64), np.zeros(2, dtype=np.float64)
        _check(self._lib.p2gpu_witness_plan_info(self._h, counts.ctypes.data, ms.ctypes.data))
        out = dict(zip(("ops", "levels", "widest_level", "slots", "seeds"), (int(x) for x in counts)))
        out.update(compile_ms=float(ms[0]), walk_ms=float(ms[1]))
        return out

    def export(self):
        """``p2gpu_witness_plan_export``: (cell_slot [num_routed_wires][degree] uint32, ops [n_ops] uint64, level_off
        [levels + 1] uint32), the plan's device arrays as numpy arrays."""
        sizes = (ctypes.c_size_t * 3)()
        _check(self._lib.p2gpu_witness_plan_export(self._h, None, None, None, sizes))
        cell_slot = np.zeros(sizes[0], dtype=np.uint32)
        ops = np.zeros(max(1, sizes[1]), dtype=np.uint64)
        level_off = np.zeros(sizes[2], dtype=np.uint32)
        _check(self._lib.p2gpu_witness_plan_export(self._h, cell_slot.ctypes.data, ops.ctypes.data, level_off.ctypes.data, sizes))
        return cell_slot.reshape(self._cd.num_routed_wires, self._cd.degree), ops[:sizes[1]], level_off

    def export_generators(self):
        """``p2gpu_witness_plan_export_generators``: the plan's generator table [generators][4] uint32, cell key
        (col << degree_bits | row) | bit 31 = this generator writes the cell's slot."""
        count = ctypes.c_size_t()
        _check(self._lib.p2gpu_witness_plan_export_generators(self._h, None, ctypes.byref(count)))
        table = np.zeros((count.value, 4), dtype=np.uint32)
        if count.value:
            _check(self._lib.p2gpu_witness_plan_export_generators(self._h, table.ctypes.data, ctypes.byref(count)))
        return table

    def export_generators_v(self):
        """``p2gpu_witness_plan_export_generators_v``: (off [generators + 1] uint32, table [off[-1]] uint32) of any plan:
        generator g's table words are table[off[g]:off[g + 1]], one per cell in list order, cell key | bit 31 = this naming
        writes the cell's slot."""
        sizes = (ctypes.c_size_t * 2)()
        _check(self._lib.p2gpu_witness_plan_export_generators_v(self._h, None, None, sizes))
        off, table = np.zeros(sizes[0] + 1, dtype=np.uint32), np.zeros(max(1, sizes[1]), dtype=np.uint32)
        _check(self._lib.p2gpu_witness_plan_export_generators_v(self._h, off.ctypes.data, table.ctypes.data, sizes))
        return off, table[:sizes[1]]

    def generate(self, values):
        """``p2gpu_generate_witness``: the wire matrix [num_wires][degree] as an int64 tensor on the circuit's GPU."""
        import torch

        v = self._values(values)
        cd = self._cd
        out = torch.empty((cd.num_wires, cd.degree), dtype=torch.int64, device=f"cuda:{cd.device_index()}")
        _check(self._lib.p2gpu_generate_witness(self._h, v.ctypes.data if v.size else None, ctypes.c_void_p(out.data_ptr())))
        return out

    def generate_batch(self, values_list):
        """``p2gpu_generate_witness_batch``: one level walk for all of `values_list`.  Returns (the wire matrices
        [B][num_wires][degree] as an int64 tensor on the circuit's GPU, the status per member: 0 or -5, the (row, col) of a
        failing member's first contradiction or None).  A failing member does not raise; the others' matrices are complete."""
        import torch

        rows = [self._values(v) for v in values_list]
        if not rows:
            raise P2GpuError(-7, "generate_batch needs at least one set of values")
        v = np.ascontiguousarray(np.stack(rows))
        cd = self._cd
        out = torch.empty((len(rows), cd.num_wires, cd.degree), dtype=torch.int64, device=f"cuda:{cd.device_index()}")
        status = np.zeros(len(rows), dtype=np.intc)
        bad = np.zeros((len(rows), 2), dtype=np.uint32)
        rc = self._lib.p2gpu_generate_witness_batch(self._h, v.ctypes.data if v.size else None, len(rows), ctypes.c_void_p(out.data_ptr()),
                                                    status.ctypes.data, bad.ctypes.data)
        if rc != -5:
            _check(rc)
        return out, [int(s) for s in status], [(int(r), int(c)) if s else None for s, (r, c) in zip(status, bad)]

    def _prove_batch_one_call(self, values_list, public_inputs):
        """``p2gpu_prove_seeds_batch``: (per member the proof or the error, the walk's cell per member or None)."""
        rows = [self._values(v) for v in values_list]
        if not rows:
            raise P2GpuError(-7, "prove_batch needs at least one set of values")
        v = np.ascontiguousarray(np.stack(rows))
        cd = self._cd
        pis, n_pi = cd._batch_pis(len(rows), public_inputs)
        out = np.zeros((len(rows), cd._bound), dtype=np.uint8)
        status = np.zeros(len(rows), dtype=np.intc)
        bad = np.full((len(rows), 2), 0xFFFFFFFF, dtype=np.uint32)
        rc = self._lib.p2gpu_prove_seeds_batch(self._h, v.ctypes.data if v.size else None, len(rows), pis.ctypes.data, n_pi, out.ctypes.data,
                                               status.ctypes.data, bad.ctypes.data)
        res = cd._batch_results(rc, out, status)
        cells = [(int(r), int(c)) if int(r) != 0xFFFFFFFF else None for r, c in bad]
        for b, cell in enumerate(cells):
            if cell is not None:
                res[b] = P2GpuError(int(status[b]), "unsatisfiable: witness %d of the batch contradicts itself at cell (row %d, column %d)" % (b, *cell))
        return res, cells

    def prove_batch(self, values_list, public_inputs=None, verify=False, one_call=False):
        """`generate_batch`, then the resident proof (``CircuitData.prove`` on the member's matrix) of every good member, in
        order.  `public_inputs`: one list per member.  Returns per member the ``ProofWithPublicInputs``, or the ``P2GpuError``
        a lone ``prove`` would have raised.  verify=True: also one ``CircuitData.verify_batch`` over the proofs just made;
        returns (that list, the :class:`VerifyReport` per member, None where there is no proof).  one_call=True: the walk and
        every proof in one ``p2gpu_prove_seeds_batch`` (small circuits: ``CircuitData.prove_batch``) -- the same proofs."""
        if one_call:
            out, _ = self._prove_batch_one_call(values_list, public_inputs)
        else:
            wires, status, bad = self.generate_batch(values_list)
            out = []
            for b, st in enumerate(status):
                if st:
                    out.append(P2GpuError(st, "unsatisfiable: witness %d of the batch contradicts itself at cell (row %d, column %d)" % (b, *bad[b])))
                    continue
                try:
                    out.append(self._cd.prove(wires[b], public_inputs[b] if public_inputs is not None else ()))
                except P2GpuError as e:
                    out.append(e)
        if not verify:
            return out
        made = [i for i, o in enumerate(out) if not isinstance(o, P2GpuError)]
        reports = [None] * len(out)
        if made:
            for i, r in zip(made, self._cd.verify_batch([out[i] for i in made])):
                reports[i] = r
        return out, reports

    def check(self, values, public_inputs=(), details=False):
        """``p2gpu_check_seeds``: generate into the handle's own buffer, then ``CircuitData.check_witness`` on it: does the level
        walk's output satisfy the gates and the copies?  A witness the walk itself refuses raises as :meth:`generate` does."""
        v = self._values(values)
        return self._cd._check_call(lambda pis, n_pi, rep, st, fl: self._lib.p2gpu_check_seeds(
            self._h, v.ctypes.data if v.size else None, pis, n_pi, rep, st, fl), 1, [public_inputs], details)[0]

    def check_batch(self, values_list, public_inputs=None, details=False):
        """`generate_batch`, then one ``p2gpu_check_witness_dev`` over all its matrices.  Returns ([WitnessReport], the wire
        matrices, the walk's status per member); the report of a member the walk refused describes the incomplete matrix."""
        wires, status, _ = self.generate_batch(values_list)
        return self._cd.check_witness_batch(wires, public_inputs, details), wires, status

    def prove(self, values, public_inputs=()):
        """``p2gpu_prove_seeds``: generate into the handle's own buffer, then the resident proof path."""
        v = self._values(values)
        pis = _u64(np.array(list(public_inputs), dtype=np.uint64))
        out = np.zeros(self._cd._bound, dtype=np.uint8)
        plen = ctypes.c_size_t(out.nbytes)
        tm = _Timings()
        _check(self._lib.p2gpu_prove_seeds(self._h, v.ctypes.data if v.size else None, pis.ctypes.data, len(pis), out.ctypes.data,
                                           ctypes.byref(plen), ctypes.byref(tm)))
        return ProofWithPublicInputs(out[:plen.value].tobytes(), {f: getattr(tm, f) for f, _ in _Timings._fields_})

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.p2gpu_witness_plan_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _verify(lib, handle, proof):
    data = proof.to_bytes() if hasattr(proof, "to_bytes") else bytes(proof)
    buf = np.frombuffer(data, dtype=np.uint8)
    _check(lib.p2gpu_verify(handle, buf.ctypes.data if buf.size else None, buf.size))


def _batch_bytes(proofs):
    """(the members' bytes, back to back; offsets [batch + 1]; the members)"""
    datas = [p.to_bytes() if hasattr(p, "to_bytes") else bytes(p) for p in proofs]
    offsets = np.zeros(len(datas) + 1, dtype=np.uintp)
    offsets[1:] = np.cumsum([len(d) for d in datas], dtype=np.uint64)
    return np.frombuffer(b"".join(datas) or b"\0", dtype=np.uint8), offsets, datas


def _verify_batch(lib, handle, proofs, device, compressed=False):
    buf, offsets, datas = _batch_bytes(proofs)
    reports = (_VerifyReport * max(len(datas), 1))()
    if compressed:
        fn = lib.p2gpu_verify_batch_compressed if device else lib.p2gpu_verify_batch_compressed_host
    else:
        fn = lib.p2gpu_verify_batch if device else lib.p2gpu_verify_batch_host
    rc = fn(handle, buf.ctypes.data, offsets.ctypes.data, len(datas), ctypes.byref(reports))
    if rc not in (0, -9):
        _check(rc)
    text = ctypes.create_string_buffer(400)
    out = []
    for r in reports[:len(datas)]:
        _check(lib.p2gpu_verify_reason(ctypes.byref(r), text, len(text)))
        out.append(VerifyReport(r, text.value.decode(errors="replace")))
    return out


def _decompress_batch(lib, handle, proofs):
    """``p2gpu_proof_decompress_batch``: per member its ProofWithPublicInputs, or the P2GpuError the lone ``decompress`` raises."""
    buf, offsets, datas = _batch_bytes(proofs)
    want = int(lib.p2gpu_proof_size_bound(handle))
    out = np.zeros((max(len(datas), 1), want), dtype=np.uint8)
    status = np.zeros(max(len(datas), 1), dtype=np.int32)
    _check(lib.p2gpu_proof_decompress_batch(handle, buf.ctypes.data, offsets.ctypes.data, len(datas), out.ctypes.data, status.ctypes.data))
    res = []
    for i, data in enumerate(datas):
        if status[i] == 0:
            res.append(ProofWithPublicInputs(out[i].tobytes()))
            continue
        try:  # (the words of that member's error: the host's lone call says them)
            _convert(lib.p2gpu_proof_decompress, handle, data)
            res.append(P2GpuError(int(status[i]), "malformed proof"))
        except P2GpuError as e:
            res.append(e)
    return res


def _convert(fn, handle, data):
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    n = ctypes.c_size_t(0)
    _check(fn(handle, buf.ctypes.data if buf.size else None, buf.size, None, ctypes.byref(n)))
    out = np.zeros(max(n.value, 1), dtype=np.uint8)
    _check(fn(handle, buf.ctypes.data if buf.size else None, buf.size, out.ctypes.data, ctypes.byref(n)))
    return out[:n.value].tobytes()


class _ProofFormats:
    """`proof.compress(..)` / `.decompress(..)` / `verify_compressed` of the reference's prove and
    verify actions (prove_action.rs:75-78, verify_action.rs:11-17), on either kind of handle."""

    def compress(self, proof):
        data = proof.to_bytes() if hasattr(proof, "to_bytes") else bytes(proof)
        return _convert(self._lib.p2gpu_proof_compress, self._h, data)

    def decompress(self, compressed):
        return ProofWithPublicInputs(_convert(self._lib.p2gpu_proof_decompress, self._h, compressed))

    def verify_compressed(self, compressed):
        buf = np.frombuffer(bytes(compressed), dtype=np.uint8)
        _check(self._lib.p2gpu_verify_compressed(self._h, buf.ctypes.data if buf.size else None, buf.size))

    def to_plonky2_bytes(self):
        """``verifier_data.to_bytes(&BackendGateSerializer)``: the VK file `write_vk` stores
        (write_vk_action.rs:77-80).  UNPINNED restatement of plonky2's serialization (include/p2gpu.h)."""
        n = ctypes.c_size_t(0)
        _check(self._lib.p2gpu_circuit_export_vk_plonky2(self._h, None, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        _check(self._lib.p2gpu_circuit_export_vk_plonky2(self._h, out.ctypes.data, ctypes.byref(n)))
        return out[:n.value].tobytes()


# the prover handle offers the same three conversions
CircuitData.compress = _ProofFormats.compress
CircuitData.decompress = _ProofFormats.decompress
CircuitData.verify_compressed = _ProofFormats.verify_compressed
CircuitData.to_plonky2_vk_bytes = _ProofFormats.to_plonky2_bytes


class VerifierCircuitData(_ProofFormats):
    """Verifier-only handle (``VerifierCircuitData`` of the reference's verify action,
    plonky2-backend/src/actions/verify_action.rs:11-17).  Host code only: works without a GPU."""

    def __init__(self, blob):
        lib = load_library()
        self._lib = lib
        self._blob = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8))
        self._h = ctypes.c_void_p()
        _check(lib.p2gpu_verifier_create(self._blob.ctypes.data, self._blob.nbytes, ctypes.byref(self._h)))
        self._read_header()

    @classmethod
    def from_plonky2_bytes(cls, vk, hasher=0):
        """``VerifierCircuitData::from_bytes(buffer, &BackendGateSerializer)`` of the reference's verify action
        (noir_and_plonky2_serialization.rs:16-22).  UNPINNED restatement of plonky2's serialization."""
        self = cls.__new__(cls)
        lib = load_library()
        self._lib = lib
        buf = np.ascontiguousarray(np.frombuffer(bytes(vk), dtype=np.uint8))
        self._h = ctypes.c_void_p()
        _check(lib.p2gpu_verifier_create_plonky2(buf.ctypes.data if buf.size else None, buf.size, int(hasher), ctypes.byref(self._h)))
        n = ctypes.c_size_t(0)
        _check(lib.p2gpu_circuit_export_vk(self._h, None, ctypes.byref(n)))
        self._blob = np.zeros(n.value, dtype=np.uint8)
        _check(lib.p2gpu_circuit_export_vk(self._h, self._blob.ctypes.data, ctypes.byref(n)))
        self._read_header()
        return self

    def _read_header(self):
        hdr = self._blob[:256].view(np.uint32)
        self.degree_bits = int(hdr[2])
        self.cap_height = int(hdr[10])
        self.num_public_inputs = int(hdr[24])

    def to_bytes(self):
        return self._blob.tobytes()

    def hash_bytes(self):
        return int(self._lib.p2gpu_circuit_hash_bytes(self._h))

    def circuit_digest(self):
        out = np.zeros(self.hash_bytes(), dtype=np.uint8)
        _check(self._lib.p2gpu_circuit_digest(self._h, out.ctypes.data))
        return out.tobytes()

    def constants_sigmas_cap(self):
        out = np.zeros(self.hash_bytes() << self.cap_height, dtype=np.uint8)
        _check(self._lib.p2gpu_circuit_cap(self._h, out.ctypes.data))
        return out.tobytes()

    def verify(self, proof):
        _verify(self._lib, self._h, proof)

    def verify_batch(self, proofs, device=True):
        """One :class:`VerifyReport` per proof.  device=True: ``p2gpu_verify_batch`` on the first device of ``init`` (the
        handle keeps no device state: its few kilobytes are uploaded per call); device=False: ``p2gpu_verify_batch_host``, the
        same checks in a plain loop on this thread.  An invalid proof raises nothing; P2GpuError is for argument and device
        errors (without a GPU, device=True raises: there is no silent fall-back)."""
        return _verify_batch(self._lib, self._h, proofs, device)

    def verify_batch_compressed(self, proofs, device=True):
        """``verify_batch`` for compressed proofs (the on-disk format): device=True: ``p2gpu_verify_batch_compressed``, the
        decompression on the device too; device=False: ``p2gpu_verify_batch_compressed_host``, the same core in a plain loop on
        this thread.  The verdict of each proof is ``verify_compressed``'s."""
        return _verify_batch(self._lib, self._h, proofs, device, compressed=True)

    def decompress_batch(self, proofs):
        """``p2gpu_proof_decompress_batch``: the device's decompression of each compressed proof, read back -- per member a
        :class:`ProofWithPublicInputs` with the bytes of ``decompress``, or the :class:`P2GpuError` ``decompress`` raises."""
        return _decompress_batch(self._lib, self._h, proofs)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.p2gpu_circuit_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- build(): the GPU-free precompute + circuit creation -----------------------
class _BuildParams(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint32) for k in ("degree_bits", "num_wires", "num_routed_wires", "num_challenges", "quotient_degree_factor",
                                                "rate_bits", "cap_height", "proof_of_work_bits", "num_query_rounds", "num_public_inputs")]


class _GateDecl(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("p", ctypes.c_uint32 * 4), ("degree", ctypes.c_uint32), ("num_constants", ctypes.c_uint32)]


def _build_args(degree_bits, gates, row_gate, row_constants, copies, num_public_inputs, num_wires, num_routed_wires, num_challenges,
                quotient_degree_factor, rate_bits, cap_height, proof_of_work_bits, num_query_rounds):
    """The ctypes / numpy forms of what ``build_blob`` and ``CircuitData.build`` hand to the library."""
    bp = _BuildParams(degree_bits, num_wires, num_routed_wires, num_challenges, quotient_degree_factor, rate_bits, cap_height,
                      proof_of_work_bits, num_query_rounds, num_public_inputs)
    gd = (_GateDecl * len(gates))()
    for i, (kind, ps, deg, nk) in enumerate(gates):
        gd[i].kind, gd[i].degree, gd[i].num_constants = kind, deg, nk
        for j, v in enumerate(tuple(ps) + (0,) * (4 - len(ps))):
            gd[i].p[j] = v
    rg = np.ascontiguousarray(row_gate, dtype=np.uint32)
    rc = np.ascontiguousarray(row_constants, dtype=np.uint64)
    cp = np.ascontiguousarray(copies, dtype=np.uint32).reshape(-1, 4)
    if rg.size != 1 << degree_bits:
        raise P2GpuError(-7, "row_gate must have 2^degree_bits entries")
    return bp, gd, rg, rc, cp


def build_blob(degree_bits, gates, row_gate, row_constants, copies, num_public_inputs=0, num_wires=234, num_routed_wires=80,
               num_challenges=2, quotient_degree_factor=8, rate_bits=3, cap_height=4, proof_of_work_bits=16, num_query_rounds=28):
    """``builder.build::<C>()`` minus the GPU part (circuit_translation/mod.rs:80-82): selector columns and groups,
    sigma polynomials from the copy constraints, k_is, FRI arities -> circuit blob (p2gpu_build_blob).
    gates: [(kind, (p0, p1, p2, p3), degree, num_constants)] sorted by (degree, id) like CommonCircuitData.gates;
    row_gate[n]; row_constants[max num_constants][n]; copies[m][4] = (row_a, col_a, row_b, col_b).
    ``CircuitData(build_blob(...))`` then commits constants and sigmas on the GPU and derives the digest."""
    lib = load_library()
    lib.p2gpu_build_blob.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    bp, gd, rg, rc, cp = _build_args(degree_bits, gates, row_gate, row_constants, copies, num_public_inputs, num_wires, num_routed_wires,
                                     num_challenges, quotient_degree_factor, rate_bits, cap_height, proof_of_work_bits, num_query_rounds)
    ln = ctypes.c_size_t(0)
    args = [ctypes.byref(bp), gd, len(gates), rg.ctypes.data, rc.ctypes.data if rc.size else None, cp.ctypes.data if cp.size else None, len(cp)]
    _check(lib.p2gpu_build_blob(*args, None, ctypes.byref(ln)))
    out = np.zeros(ln.value, dtype=np.uint8)
    _check(lib.p2gpu_build_blob(*args, out.ctypes.data, ctypes.byref(ln)))
    return out[:ln.value]


# ---- stage-level operators ---------------------------------------------------
def ifft_batch(vals):
    """PolynomialValues::ifft on every row of `vals` [ncols][2^d]."""
    lib = load_library()
    v = _u64(vals)
    ncols, n = v.shape
    d = n.bit_length() - 1
    out = np.zeros_like(v)
    _check(lib.p2gpu_ifft_batch(v.ctypes.data, ncols, d, out.ctypes.data))
    return out


def lde_batch(coeffs, rate_bits=3):
    """PolynomialCoeffs::lde(rate_bits).coset_fft(7) on every row of `coeffs`."""
    lib = load_library()
    c = _u64(coeffs)
    ncols, n = c.shape
    d = n.bit_length() - 1
    out = np.zeros((ncols, n << rate_bits), dtype=np.uint64)
    _check(lib.p2gpu_lde_batch(c.ctypes.data, ncols, d, rate_bits, out.ctypes.data))
    return out


def commit_values(vals, rate_bits=3, cap_height=4):
    """PolynomialBatch::from_values(...).merkle_tree.cap as bytes (2^cap_height x 25)."""
    lib = load_library()
    v = _u64(vals)
    ncols, n = v.shape
    d = n.bit_length() - 1
    out = np.zeros(25 << cap_height, dtype=np.uint8)
    _check(lib.p2gpu_commit_values(v.ctypes.data, ncols, d, rate_bits, cap_height, out.ctypes.data))
    return out.tobytes()


def field_selftest(a, b):
    """Mismatch counters of the device field primitives against the portable code on the word pairs (a[i], b[i])."""
    lib = load_library()
    x = np.ascontiguousarray(a, dtype=np.uint64)
    y = np.ascontiguousarray(b, dtype=np.uint64)
    assert x.shape == y.shape and x.ndim == 1
    bad = np.zeros(16, dtype=np.uint64)
    _check(lib.p2gpu_field_selftest16(x.ctypes.data, y.ctypes.data, x.size, bad.ctypes.data))
    return bad


# p2gpu_forms_selftest: form -> (number, words per case of in, aux, out)
FORMS = {"mds": (0, 12, 0, 12), "sbox": (1, 1, 0, 2), "fused3": (2, 12, 2, 12), "fused2": (3, 12, 2, 12), "permute": (4, 12, 0, 12),
         "coop": (5, 12, 4, 12), "smalldot": (6, 12, 12, 2), "horner": (7, 32, 32, 1), "acc160": (8, 2, 1, 1), "range4": (9, 1, 0, 1)}


def forms_selftest(form, inp, aux=None):
    """The raw device words of one device-only form (include/p2gpu.h p2gpu_forms_selftest) on the cases `inp` [n][in words]
    with `aux` [n][aux words]; [n][out words].  Nothing is compared here."""
    lib = load_library()
    num, in_w, aux_w, out_w = FORMS[form]
    x = np.ascontiguousarray(inp, dtype=np.uint64).reshape(-1, in_w)
    n = x.shape[0]
    a = None
    if aux is not None:
        a = np.ascontiguousarray(aux, dtype=np.uint64).reshape(-1, aux_w)
        assert a.shape[0] == n
    out = np.zeros((n, out_w), dtype=np.uint64)
    _check(lib.p2gpu_forms_selftest(num, x.ctypes.data, n, a.ctypes.data if a is not None else None, out.ctypes.data))
    return out


def hash_rows(rows):
    """KeccakHash<25>::hash_or_noop of every row."""
    lib = load_library()
    r = _u64(rows)
    n_rows, row_len = r.shape
    out = np.zeros(25 * n_rows, dtype=np.uint8)
    _check(lib.p2gpu_hash_rows(r.ctypes.data, n_rows, row_len, out.ctypes.data))
    return out.reshape(n_rows, 25)
