"""ctypes mirror of include/icicle_snark_hip.h (the reference's extern "C" surface for the Groth16 path).

Names follow the reference's Rust wrappers so that tests read like theirs:
``msm`` (icicle-core/src/msm/mod.rs:106-154), ``ntt`` / ``initialize_domain`` / ``release_domain`` /
``get_root_of_unity`` (ntt/mod.rs:202-216,290-305), ``mul_scalars`` / ``sub_scalars`` / ``add_scalars``
(vec_ops/mod.rs:233-245), ``from_mont`` / ``to_mont`` (field.rs:379-398, curve.rs:140-154), ``DeviceVec``
(icicle-runtime/src/memory.rs), ``IcicleStream`` (stream.rs).

There is NO fallback of any kind here: if the shared library is missing or no HIP device is present the
calls raise.  Arrays are numpy uint64 with a trailing dimension of 4 (32-byte little-endian elements).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libicicle_snark_hip.so")
# The prover overlaps six streams; the HIP runtime's default of four hardware queues makes two of them serialise
# (csrc/runtime.cpp does the same when the library is loaded; set here too so that it also precedes any other DSO
# of this process that initialises the HIP runtime first, e.g. RCCL).
os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")

SUCCESS = 0
ERRORS = ["SUCCESS", "INVALID_DEVICE", "OUT_OF_MEMORY", "INVALID_POINTER", "ALLOCATION_FAILED", "DEALLOCATION_FAILED",
          "COPY_FAILED", "SYNCHRONIZATION_FAILED", "STREAM_CREATION_FAILED", "STREAM_DESTRUCTION_FAILED",
          "API_NOT_IMPLEMENTED", "INVALID_ARGUMENT", "BACKEND_LOAD_FAILED", "LICENSE_CHECK_ERROR", "UNKNOWN_ERROR"]


class IcicleError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        name = ERRORS[code] if 0 <= code < len(ERRORS) else str(code)
        super().__init__(f"eIcicleError::{name} {what}".strip())


class Device(C.Structure):
    _fields_ = [("type", C.c_char * 64), ("id", C.c_int)]


class MSMConfig(C.Structure):
    _fields_ = [("stream", C.c_void_p), ("precompute_factor", C.c_int), ("c", C.c_int), ("bitsize", C.c_int),
                ("batch_size", C.c_int), ("are_points_shared_in_batch", C.c_bool), ("are_scalars_on_device", C.c_bool),
                ("are_scalars_montgomery_form", C.c_bool), ("are_points_on_device", C.c_bool),
                ("are_points_montgomery_form", C.c_bool), ("are_results_on_device", C.c_bool), ("is_async", C.c_bool),
                ("ext", C.c_void_p)]

    @staticmethod
    def default():
        return MSMConfig(None, 1, 0, 0, 1, True, False, False, False, False, False, False, None)


class NTTConfig(C.Structure):
    _fields_ = [("stream", C.c_void_p), ("coset_gen", C.c_uint32 * 8), ("batch_size", C.c_int), ("columns_batch", C.c_bool),
                ("ordering", C.c_int), ("are_inputs_on_device", C.c_bool), ("are_outputs_on_device", C.c_bool),
                ("is_async", C.c_bool), ("ext", C.c_void_p)]

    @staticmethod
    def default():
        one = (C.c_uint32 * 8)(1, 0, 0, 0, 0, 0, 0, 0)
        return NTTConfig(None, one, 1, False, 0, False, False, False, None)


class NTTInitDomainConfig(C.Structure):
    _fields_ = [("stream", C.c_void_p), ("is_async", C.c_bool), ("ext", C.c_void_p)]


class VecOpsConfig(C.Structure):
    _fields_ = [("stream", C.c_void_p), ("is_a_on_device", C.c_bool), ("is_b_on_device", C.c_bool),
                ("is_result_on_device", C.c_bool), ("is_async", C.c_bool), ("batch_size", C.c_int),
                ("columns_batch", C.c_bool), ("ext", C.c_void_p)]

    @staticmethod
    def default():
        return VecOpsConfig(None, False, False, False, False, 1, False, None)


# every symbol include/icicle_snark_hip.h declares (checked by tests/test_abi.py)
DECLARED_SYMBOLS = """
icicle_load_backend icicle_load_backend_from_env_or_default icicle_set_device icicle_set_default_device
icicle_get_active_device icicle_is_host_memory icicle_is_active_device_memory icicle_get_device_count
icicle_is_device_available icicle_get_registered_devices icicle_malloc icicle_malloc_async icicle_free icicle_free_async
icicle_get_available_memory icicle_memset icicle_memset_async icicle_copy icicle_copy_async icicle_copy_to_host
icicle_copy_to_host_async icicle_copy_to_device icicle_copy_to_device_async icicle_create_stream icicle_destroy_stream
icicle_stream_synchronize icicle_device_synchronize icicle_get_device_properties
create_config_extension destroy_config_extension config_extension_set_int config_extension_set_bool
config_extension_get_int config_extension_get_bool clone_config_extension
bn254_generate_scalars bn254_add bn254_sub bn254_mul bn254_inv bn254_pow bn254_from_u32
bn254_eq bn254_ecadd bn254_ecsub bn254_mul_scalar bn254_to_affine bn254_from_affine bn254_generator bn254_is_on_curve
bn254_base_field_from_u32 bn254_g2_eq bn254_g2_ecadd bn254_g2_ecsub bn254_g2_mul_scalar bn254_g2_to_affine
bn254_g2_from_affine bn254_g2_generator bn254_g2_is_on_curve bn254_g2_base_field_from_u32
bn254_vector_add bn254_vector_sub bn254_vector_mul bn254_scalar_convert_montgomery
bn254_affine_convert_montgomery bn254_g2_affine_convert_montgomery
bn254_ntt bn254_ntt_init_domain bn254_ntt_release_domain bn254_get_root_of_unity bn254_get_root_of_unity_from_domain
bn254_msm bn254_g2_msm bn254_pairing
bn254_vector_div bn254_vector_accumulate bn254_vector_sum bn254_vector_product bn254_scalar_add_vec bn254_scalar_sub_vec
bn254_scalar_mul_vec bn254_projective_convert_montgomery bn254_g2_projective_convert_montgomery
bn254_msm_precompute_bases bn254_g2_msm_precompute_bases
bn254_pairing_target_field_add bn254_pairing_target_field_sub bn254_pairing_target_field_mul bn254_pairing_target_field_inv
bn254_pairing_target_field_pow bn254_pairing_target_field_from_u32 bn254_pairing_target_field_generate_scalars
icicle_snark_last_error icicle_snark_g1_generator_mul icicle_snark_g2_generator_mul icicle_snark_last_msm_timings
icicle_snark_msm_profile icicle_snark_microbench icicle_snark_pmc_probes icicle_snark_access_probes
icicle_snark_pairing_batch icicle_snark_pairing_product icicle_snark_msm_segmented
""".split()

_lib = None


def lib():
    """Load the C-ABI library. Raises if it has not been built — there is no Python/CPU substitute."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `make` (hipcc --offload-arch=gfx950); "
                              "this package has no CPU fallback")
        _lib = C.CDLL(LIB_PATH)
        _lib.icicle_snark_last_error.restype = C.c_char_p
        _lib.groth16_last_error.restype = _lib.groth16_verify_last_error.restype = C.c_char_p
        _lib.groth16_cache_manager_new.restype = C.c_void_p
        _lib.groth16_zkey_export_vk.restype = C.c_int64
        _lib.groth16_verify_combined_coefficients.restype = _lib.groth16_vkset_free.restype = None
        for n in ("bn254_eq", "bn254_g2_eq", "bn254_is_on_curve", "bn254_g2_is_on_curve"):
            getattr(_lib, n).restype = C.c_bool
    return _lib


def check(rc, what=""):
    if rc != SUCCESS:
        msg = lib().icicle_snark_last_error()
        raise IcicleError(rc, f"{what}: {msg.decode() if msg else ''}")


def set_device(dev_type: str = "HIP", dev_id: int = 0):
    """try_load_and_set_backend_device — src/lib.rs:25-31"""
    if dev_type != "CPU":
        check(lib().icicle_load_backend_from_env_or_default(), "load_backend")
    d = Device(dev_type.encode(), dev_id)
    check(lib().icicle_set_device(C.byref(d)), f"set_device({dev_type},{dev_id})")


def ptr_of(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data_as(C.c_void_p)
    if isinstance(a, DeviceVec):
        return C.c_void_p(a.ptr)
    if isinstance(a, int):
        return C.c_void_p(a)
    raise TypeError(type(a))


def _on_dev(a):
    return isinstance(a, (DeviceVec, int))


class IcicleStream:
    """icicle-runtime/src/stream.rs"""

    def __init__(self, handle=None):
        if handle is None:
            h = C.c_void_p()
            check(lib().icicle_create_stream(C.byref(h)), "create_stream")
            self.handle, self._own = h.value, True
        else:
            self.handle, self._own = handle, False

    def synchronize(self):
        check(lib().icicle_stream_synchronize(C.c_void_p(self.handle)), "stream_synchronize")

    def destroy(self):
        if self._own and self.handle is not None:
            check(lib().icicle_destroy_stream(C.c_void_p(self.handle)), "destroy_stream")
            self.handle = None


class DeviceVec:
    """A device allocation of `nbytes` bytes (icicle-runtime/src/memory.rs:351-417). Slices share the parent."""

    def __init__(self, nbytes: int, stream: IcicleStream | None = None, _ptr=None, _parent=None):
        self.nbytes = nbytes
        self._parent = _parent
        if _ptr is not None:
            self.ptr = _ptr
            return
        p = C.c_void_p()
        if stream is None:
            check(lib().icicle_malloc(C.byref(p), C.c_size_t(max(nbytes, 1))), "malloc")
        else:
            check(lib().icicle_malloc_async(C.byref(p), C.c_size_t(max(nbytes, 1)), C.c_void_p(stream.handle)), "malloc_async")
        self.ptr = p.value

    @staticmethod
    def from_host(a: np.ndarray, stream: IcicleStream | None = None) -> "DeviceVec":
        a = np.ascontiguousarray(a)
        d = DeviceVec(a.nbytes, stream)
        d.copy_from_host(a, stream)
        return d

    def slice(self, byte_off: int, nbytes: int) -> "DeviceVec":
        assert 0 <= byte_off and byte_off + nbytes <= self.nbytes
        return DeviceVec(nbytes, _ptr=self.ptr + byte_off, _parent=self)

    def copy_from_host(self, a: np.ndarray, stream: IcicleStream | None = None):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        if stream is None:
            check(lib().icicle_copy_to_device(C.c_void_p(self.ptr), ptr_of(a), C.c_size_t(a.nbytes)), "copy_to_device")
        else:
            check(lib().icicle_copy_to_device_async(C.c_void_p(self.ptr), ptr_of(a), C.c_size_t(a.nbytes), C.c_void_p(stream.handle)), "copy_to_device_async")

    def to_host(self, shape, dtype=np.uint64, stream: IcicleStream | None = None) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        if stream is None:
            check(lib().icicle_copy_to_host(ptr_of(out), C.c_void_p(self.ptr), C.c_size_t(out.nbytes)), "copy_to_host")
        else:
            check(lib().icicle_copy_to_host_async(ptr_of(out), C.c_void_p(self.ptr), C.c_size_t(out.nbytes), C.c_void_p(stream.handle)), "copy_to_host_async")
            stream.synchronize()
        return out

    def free(self):
        if self._parent is None and self.ptr:
            check(lib().icicle_free(C.c_void_p(self.ptr)), "free")
            self.ptr = 0


# --------------------------------------------------------------------------------------------- vec ops
def _vec_cfg(a, b, out, stream, is_async, batch_size=1, columns_batch=False):
    """the VecOpsConfig of one call: where a, b and out live (None: the host), the stream, the batch"""
    cfg = VecOpsConfig.default()
    cfg.is_a_on_device, cfg.is_b_on_device, cfg.is_result_on_device = _on_dev(a), _on_dev(b), _on_dev(out)
    cfg.is_async, cfg.batch_size, cfg.columns_batch = is_async, batch_size, columns_batch
    cfg.stream = stream.handle if stream else None
    return cfg


def _vec_op(name, a, b, out, n, stream, is_async):
    cfg = _vec_cfg(a, b, out, stream, is_async)
    check(getattr(lib(), name)(ptr_of(a), ptr_of(b), C.c_uint64(n), C.byref(cfg), ptr_of(out)), name)


def _n_of(a):
    return a.size // 4 if isinstance(a, np.ndarray) else a.nbytes // 32


def mul_scalars(a, b, out=None, stream=None, is_async=False):
    if out is None:
        out = np.empty((_n_of(a), 4), dtype=np.uint64)
    _vec_op("bn254_vector_mul", a, b, out, _n_of(a), stream, is_async)
    return out


def sub_scalars(a, b, out=None, stream=None, is_async=False):
    if out is None:
        out = np.empty((_n_of(a), 4), dtype=np.uint64)
    _vec_op("bn254_vector_sub", a, b, out, _n_of(a), stream, is_async)
    return out


def add_scalars(a, b, out=None, stream=None, is_async=False):
    if out is None:
        out = np.empty((_n_of(a), 4), dtype=np.uint64)
    _vec_op("bn254_vector_add", a, b, out, _n_of(a), stream, is_async)
    return out


def vec_op2(name: str, a, b, n=None, batch_size=1, columns_batch=False, out=None, stream=None, is_async=False):
    """element-wise a ∘ b for name in add/sub/mul/div over n·batch_size elements (icicle-core vec_ops/mod.rs)"""
    total = _n_of(a)
    if out is None:
        out = np.empty((total, 4), dtype=np.uint64)
    cfg = _vec_cfg(a, b, out, stream, is_async, batch_size, columns_batch)
    n = total // batch_size if n is None else n
    check(getattr(lib(), "bn254_vector_" + name)(ptr_of(a), ptr_of(b), C.c_uint64(n), C.byref(cfg), ptr_of(out)), name)
    return out


def accumulate_scalars(a, b, stream=None, is_async=False):
    """a += b in place — vector_accumulate"""
    cfg = _vec_cfg(a, b, a, stream, is_async)
    check(lib().bn254_vector_accumulate(ptr_of(a), ptr_of(b), C.c_uint64(_n_of(a)), C.byref(cfg)), "vector_accumulate")
    return a


def scalar_vec_op(name: str, scalars, v, batch_size=1, columns_batch=False, out=None, stream=None, is_async=False):
    """out(b, i) = scalars[b] ∘ v(b, i) for name in add/sub/mul — scalar_{add,sub,mul}_vec"""
    total = _n_of(v)
    if out is None:
        out = np.empty((total, 4), dtype=np.uint64)
    cfg = _vec_cfg(scalars, v, out, stream, is_async, batch_size, columns_batch)
    check(getattr(lib(), f"bn254_scalar_{name}_vec")(ptr_of(scalars), ptr_of(v), C.c_uint64(total // batch_size), C.byref(cfg), ptr_of(out)), name)
    return out


def reduce_scalars(name: str, v, batch_size=1, columns_batch=False, stream=None, is_async=False):
    """Σ / Π of every batch vector, name in sum/product → (batch_size, 4) array"""
    out = np.empty((batch_size, 4), dtype=np.uint64)
    cfg = _vec_cfg(v, None, None, stream, is_async, batch_size, columns_batch)
    check(getattr(lib(), "bn254_vector_" + name)(ptr_of(v), C.c_uint64(_n_of(v) // batch_size), C.byref(cfg), ptr_of(out)), name)
    return out


def projective_convert_montgomery(group: str, a: np.ndarray, to_mont: bool) -> np.ndarray:
    per = 96 if group == "g1" else 192
    out = np.empty_like(a)
    cfg = _vec_cfg(a, None, out, None, False)
    name = "bn254_projective_convert_montgomery" if group == "g1" else "bn254_g2_projective_convert_montgomery"
    check(getattr(lib(), name)(ptr_of(a), C.c_size_t(a.nbytes // per), C.c_bool(to_mont), C.byref(cfg), ptr_of(out)), name)
    return out


def scalar_convert_montgomery(a, to_mont: bool, out=None, stream=None, is_async=False):
    if out is None:
        out = np.empty_like(a) if isinstance(a, np.ndarray) else a
    cfg = _vec_cfg(a, None, out, stream, is_async)
    check(lib().bn254_scalar_convert_montgomery(ptr_of(a), C.c_uint64(_n_of(a)), C.c_bool(to_mont), C.byref(cfg), ptr_of(out)), "scalar_convert_montgomery")
    return out


def affine_convert_montgomery(group: str, a, to_mont: bool, out=None, stream=None, is_async=False):
    per = 64 if group == "g1" else 128
    n = (a.nbytes if isinstance(a, (np.ndarray, DeviceVec)) else 0) // per
    if out is None:
        out = np.empty_like(a) if isinstance(a, np.ndarray) else a
    cfg = _vec_cfg(a, None, out, stream, is_async)
    name = "bn254_affine_convert_montgomery" if group == "g1" else "bn254_g2_affine_convert_montgomery"
    check(getattr(lib(), name)(ptr_of(a), C.c_uint64(n), C.c_bool(to_mont), C.byref(cfg), ptr_of(out)), name)
    return out


# --------------------------------------------------------------------------------------------- NTT
def get_root_of_unity(max_size: int) -> np.ndarray:
    out = np.zeros(4, dtype=np.uint64)
    check(lib().bn254_get_root_of_unity(C.c_uint64(max_size), ptr_of(out)), "get_root_of_unity")
    return out


def initialize_domain(root: np.ndarray, stream=None):
    cfg = NTTInitDomainConfig(stream.handle if stream else None, False, None)
    check(lib().bn254_ntt_init_domain(ptr_of(np.ascontiguousarray(root)), C.byref(cfg)), "ntt_init_domain")


def release_domain():
    check(lib().bn254_ntt_release_domain(), "ntt_release_domain")


def ntt(inp, inverse: bool, out=None, batch_size=1, size=None, stream=None, is_async=False, coset_gen=None, ordering=0, columns_batch=False):
    if size is None:
        size = _n_of(inp) // batch_size
    if out is None:
        out = np.empty_like(inp) if isinstance(inp, np.ndarray) else inp
    cfg = NTTConfig.default()
    cfg.batch_size = batch_size
    cfg.are_inputs_on_device, cfg.are_outputs_on_device = _on_dev(inp), _on_dev(out)
    cfg.is_async = is_async
    cfg.ordering = ordering
    cfg.columns_batch = columns_batch
    cfg.stream = stream.handle if stream else None
    if coset_gen is not None:
        cg = np.ascontiguousarray(coset_gen, dtype=np.uint64).view(np.uint32)
        for i in range(8):
            cfg.coset_gen[i] = int(cg[i])
    check(lib().bn254_ntt(ptr_of(inp), C.c_int(size), C.c_int(1 if inverse else 0), C.byref(cfg), ptr_of(out)), "ntt")
    return out


# --------------------------------------------------------------------------------------------- MSM
def msm(group: str, scalars, bases, out=None, stream=None, is_async=False, c=0, size=None,
        scalars_mont=False, points_mont=False, ext=None, batch_size=1, shared_points=True, precompute_factor=1, bitsize=0):
    """msm() — icicle-core/src/msm/mod.rs:106-154. Returns the projective result (3,4)/(6,4) u64 when `out` is None."""
    if size is None:
        size = _n_of(scalars) // batch_size
    host_out = out is None
    if host_out:
        out = np.zeros(((3, 4) if group == "g1" else (6, 4)) if batch_size == 1 else ((batch_size, 3, 4) if group == "g1" else (batch_size, 6, 4)), dtype=np.uint64)
    cfg = MSMConfig.default()
    cfg.c, cfg.bitsize = c, bitsize
    cfg.batch_size, cfg.are_points_shared_in_batch, cfg.precompute_factor = batch_size, shared_points, precompute_factor
    cfg.are_scalars_on_device, cfg.are_points_on_device, cfg.are_results_on_device = _on_dev(scalars), _on_dev(bases), _on_dev(out)
    cfg.are_scalars_montgomery_form, cfg.are_points_montgomery_form = scalars_mont, points_mont
    cfg.is_async = is_async
    cfg.stream = stream.handle if stream else None
    cfg.ext = ext
    name = "bn254_msm" if group == "g1" else "bn254_g2_msm"
    check(getattr(lib(), name)(ptr_of(scalars), ptr_of(bases), C.c_int(size), C.byref(cfg), ptr_of(out)), name)
    return out


def msm_precompute_bases(group: str, bases: np.ndarray, precompute_factor: int, c=0, points_mont=False, bitsize=0) -> np.ndarray:
    """msm_precompute_bases — icicle-core/src/msm/mod.rs:156-190 (host arrays in and out)"""
    per = 64 if group == "g1" else 128
    n = bases.nbytes // per
    out = np.empty((n * precompute_factor,) + bases.shape[1:], dtype=np.uint64)
    cfg = MSMConfig.default()
    cfg.c, cfg.precompute_factor, cfg.are_points_montgomery_form, cfg.bitsize = c, precompute_factor, points_mont, bitsize
    name = "bn254_msm_precompute_bases" if group == "g1" else "bn254_g2_msm_precompute_bases"
    check(getattr(lib(), name)(ptr_of(np.ascontiguousarray(bases)), C.c_int(n), C.byref(cfg), ptr_of(out)), name)
    return out


def raw_to_host(ptr: int, nbytes: int) -> bytes:
    """device memory at a raw pointer → bytes (exchange emulation in tests / the gloo fallback)"""
    buf = (C.c_uint8 * nbytes)()
    check(lib().icicle_copy_to_host(buf, C.c_void_p(ptr), C.c_size_t(nbytes)), "copy_to_host")
    return bytes(buf)


def raw_to_device(ptr: int, data: bytes):
    check(lib().icicle_copy_to_device(C.c_void_p(ptr), data, C.c_size_t(len(data))), "copy_to_device")


def last_msm_timings():
    out = (C.c_float * 4)()
    check(lib().icicle_snark_last_msm_timings(out), "last_msm_timings")
    return list(out)


def msm_profile(back: int = 0):
    """(ms[5], dict geom) of the `back`-th most recent MSM; see include/icicle_snark_hip.h."""
    ms = (C.c_float * 5)()
    geom = (C.c_uint32 * 5)()
    check(lib().icicle_snark_msm_profile(back, ms, geom), "msm_profile")
    return list(ms), dict(L=geom[0], nbuckets=geom[1], c=geom[2], W=geom[3], is_g2=bool(geom[4]))


def microbench():
    """(device-to-device copy GB/s counting read + write, v_mad_u64_u32 lane-ops/s in 10^12) measured now"""
    out = (C.c_double * 2)()
    check(lib().icicle_snark_microbench(out), "microbench")
    return float(out[0]), float(out[1])


def access_probes():
    """GB/s of 64-byte gathers, 128-byte gathers, coalesced reads, scattered 4-byte stores, coalesced 4-byte stores (2 GiB buffer), measured now"""
    out = (C.c_double * 5)()
    check(lib().icicle_snark_access_probes(out), "access_probes")
    return dict(zip(("gather64_gbps", "gather128_gbps", "stream_read_gbps", "scattered_store_gbps", "coalesced_store_gbps"), (round(float(x), 1) for x in out)))


def generator_mul(group: str, scalars: np.ndarray) -> np.ndarray:
    """out[i] = s[i]·G, affine standard form (extension; used by the zkey synthesiser)."""
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    n = scalars.shape[0]
    dims = 2 if group == "g1" else 4
    d_s = DeviceVec.from_host(scalars)
    d_o = DeviceVec(n * dims * 32)
    name = "icicle_snark_g1_generator_mul" if group == "g1" else "icicle_snark_g2_generator_mul"
    check(getattr(lib(), name)(C.c_void_p(d_s.ptr), C.c_uint64(n), None, C.c_void_p(d_o.ptr)), name)
    check(lib().icicle_device_synchronize(), "sync")
    out = d_o.to_host((n, dims, 4))
    d_s.free()
    d_o.free()
    return out


# --------------------------------------------------------------------------------------------- host FFI
def i2a(x):
    return np.frombuffer(int(x).to_bytes(32, "little"), dtype=np.uint64).copy()


def a2i(a):
    return int.from_bytes(np.ascontiguousarray(a).tobytes(), "little")


def fr_op(op: str, a: int, b: int) -> int:
    out = np.zeros(4, dtype=np.uint64)
    getattr(lib(), f"bn254_{op}")(ptr_of(i2a(a)), ptr_of(i2a(b)), ptr_of(out))
    return a2i(out)


def fr_inv(a: int) -> int:
    out = np.zeros(4, dtype=np.uint64)
    lib().bn254_inv(ptr_of(i2a(a)), ptr_of(out))
    return a2i(out)


_PRE = {"g1": "bn254_", "g2": "bn254_g2_"}
_DIMS = {"g1": (2, 3), "g2": (4, 6)}


def ec(group: str, op: str, *args):
    """host curve FFI: ecadd/ecsub(p,q), mul_scalar(p, int), to_affine(p), from_affine(a), generator()"""
    f = getattr(lib(), _PRE[group] + op)
    na, npj = _DIMS[group]
    if op in ("ecadd", "ecsub"):
        out = np.zeros((npj, 4), dtype=np.uint64)
        f(ptr_of(np.ascontiguousarray(args[0])), ptr_of(np.ascontiguousarray(args[1])), ptr_of(out))
    elif op == "mul_scalar":
        out = np.zeros((npj, 4), dtype=np.uint64)
        f(ptr_of(np.ascontiguousarray(args[0])), ptr_of(i2a(args[1])), ptr_of(out))
    elif op == "to_affine":
        out = np.zeros((na, 4), dtype=np.uint64)
        f(ptr_of(np.ascontiguousarray(args[0])), ptr_of(out))
    elif op == "from_affine":
        out = np.zeros((npj, 4), dtype=np.uint64)
        f(ptr_of(np.ascontiguousarray(args[0])), ptr_of(out))
    elif op == "generator":
        out = np.zeros((npj, 4), dtype=np.uint64)
        f(ptr_of(out))
    else:
        raise ValueError(op)
    return out


def ec_eq(group, a, b) -> bool:
    return bool(getattr(lib(), _PRE[group] + "eq")(ptr_of(np.ascontiguousarray(a)), ptr_of(np.ascontiguousarray(b))))


def ec_is_on_curve(group, a) -> bool:
    return bool(getattr(lib(), _PRE[group] + "is_on_curve")(ptr_of(np.ascontiguousarray(a))))


# --------------------------------------------------------------------------------------------- prover host
COMMITMENTS_BYTES = 576


class Timings(C.Structure):
    _fields_ = [("h2d_ms", C.c_double), ("qap_ms", C.c_double), ("msm_ms", C.c_double), ("total_ms", C.c_double)]


class CircuitInfo(C.Structure):
    _fields_ = [("n_vars", C.c_uint32), ("n_public", C.c_uint32), ("domain_size", C.c_uint32), ("n_coef", C.c_uint32),
                ("device_bytes", C.c_uint64), ("b_bases", C.c_uint32), ("shards", C.c_uint32)]


class ProverError(RuntimeError):
    pass


def _pcheck(rc, what):
    if rc != 0:
        msg = lib().groth16_last_error()
        raise ProverError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def _verify_fail(rc, what):
    raise ProverError(f"{what}: {lib().groth16_verify_last_error().decode()} (code {rc})")


def _image(data):
    """zero-copy pointer to the caller's ndarray, bytes or writable buffer (a 0.8 GB zkey must not be duplicated on the way in)"""
    return data.ctypes.data_as(C.c_void_p) if isinstance(data, np.ndarray) else C.c_char_p(data) if isinstance(data, bytes) else (C.c_char * len(data)).from_buffer(data)


def _is_path(x):
    return isinstance(x, (str, os.PathLike))


def _path_or_image(what, src, out):
    """True: src is a path and `out` the path to write to; False: src is an image, which takes no `out`"""
    if _is_path(src):
        if out is None:
            raise TypeError(f"{what}: an input path needs the path to write to")
        return True
    if out is not None:
        raise TypeError(f"{what}: `out` goes with an input path")
    return False


def _le32(value):
    return int(value).to_bytes(32, "little") if value is not None else None


def _seed32(seed, what, noun="seed"):
    """32 caller-chosen bytes as the array the C entry points take; None stays None (the library draws its own)"""
    if seed is None:
        return None
    if len(seed) != 32:
        raise ValueError(f"{what}: the {noun} is 32 bytes")
    return (C.c_uint8 * 32).from_buffer_copy(bytes(seed))


def _sized_twice(call, rep, size_field, what, check=lambda rc, what, rep: _pcheck(rc, what)):
    """call(buffer, room) sized by the library itself: a first call with no room is −3 and reports the bytes it needs, before any
    device work; the second fills a buffer of that size, which comes back"""
    rc = call(None, C.c_size_t(0))
    if rc != -3 or getattr(rep, size_field) == 0:
        check(rc, what, rep)
    size = getattr(rep, size_field)
    buf = C.create_string_buffer(size)
    check(call(buf, C.c_size_t(size)), what, rep)
    return buf


class CacheManager:
    """CacheManager — src/cache.rs:110-262 (include/groth16_prover.h)."""

    def __init__(self):
        self._h = C.c_void_p(lib().groth16_cache_manager_new())

    def close(self):
        if self._h:
            lib().groth16_cache_manager_free(self._h)
            self._h = None

    def contains(self, key: str) -> bool:
        return bool(lib().groth16_cache_contains(self._h, key.encode()))

    def load(self, key: str, zkey: bytes, device_id: int = 0, shard_rank: int = 0, shard_count: int = 1, wait_tables: bool = True):
        """groth16_cache_load.  A single-device key is usable before its fixed-base tables exist (they are built behind the
        first proofs); wait_tables=True (the default of this binding: tests and timings want the final layout) blocks until
        they are adopted, wait_tables=False returns like the C entry point does."""
        _pcheck(lib().groth16_cache_load(self._h, key.encode(), _image(zkey), C.c_size_t(len(zkey)), device_id, shard_rank, shard_count), "cache_load")
        if wait_tables:
            self.tables_ready(key, wait=True)

    def load_devices(self, key: str, zkey: bytes, device_ids):
        """one key over a GROUP of devices in this process (what groth16_prove builds for "HIP:0-7"): shard k lives on
        device_ids[k]; a device may be named several times (several shards on one GPU)."""
        ids = (C.c_int * len(device_ids))(*device_ids)
        _pcheck(lib().groth16_cache_load_devices(self._h, key.encode(), _image(zkey), C.c_size_t(len(zkey)), ids, len(device_ids)), "cache_load_devices")

    def set_budget(self, bytes_per_device: int):
        lib().groth16_cache_set_budget(self._h, C.c_uint64(bytes_per_device))

    def load_file(self, key: str, path: str, device_id: int = 0, shard_rank: int = 0, shard_count: int = 1, wait_tables: bool = True):
        _pcheck(lib().groth16_cache_load_file(self._h, key.encode(), path.encode(), device_id, shard_rank, shard_count), "cache_load_file")
        if wait_tables:
            self.tables_ready(key, wait=True)

    def load_packed(self, key: str, zkez, device_id: int = 0, shard_rank: int = 0, shard_count: int = 1, wait_tables: bool = True):
        """groth16_cache_load_packed / _file: load() from a PACKED key (zkey_pack) — the image, or a path — decoded on the GPU into
        the buffers load() fills; the entry is load()'s.  A faulty packed key raises ProverError (−2 "zkez: section S, element E:
        kind" / "zkez: coefficient E: kind") and nothing is cached.  One device only: anything but shard 0 of 1 is −3."""
        if _is_path(zkez):
            rc = lib().groth16_cache_load_packed_file(self._h, key.encode(), os.fsencode(zkez), device_id, shard_rank, shard_count)
        else:
            rc = lib().groth16_cache_load_packed(self._h, key.encode(), _image(zkez), C.c_size_t(len(zkez)), device_id, shard_rank, shard_count)
        _pcheck(rc, "cache_load_packed")
        if wait_tables:
            self.tables_ready(key, wait=True)

    def prove_zkez_files(self, witness: str, zkez: str, proof: str, public: str, device: str = "HIP"):
        """groth16_prove_zkez_files: prove() with a packed key file; a key the manager does not hold is loaded packed first"""
        _pcheck(lib().groth16_prove_zkez_files(witness.encode(), zkez.encode(), proof.encode(), public.encode(), device.encode(), self._h), "prove_zkez_files")

    def evict(self, key: str):
        lib().groth16_cache_evict(self._h, key.encode())

    def tables_ready(self, key: str, wait: bool = False) -> bool:
        """deferred fixed-base tables of a single-device key (groth16_cache_tables_ready): True once the key proves in its
        final layout; wait=True blocks until the build behind the first proofs has ended"""
        rc = lib().groth16_cache_tables_ready(self._h, key.encode(), int(wait))
        if rc < 0:
            _pcheck(rc, "cache_tables_ready")
        return rc == 1

    def info(self, key: str) -> CircuitInfo:
        ci = CircuitInfo()
        _pcheck(lib().groth16_cache_info(self._h, key.encode(), C.byref(ci)), "cache_info")
        return ci

    def group_describe(self, key: str) -> dict:
        """what the key runs on: shards, devices, exchange transport, RCCL ranks (groth16_group_describe)"""
        import json
        buf = C.create_string_buffer(2048)
        _pcheck(lib().groth16_group_describe(self._h, key.encode(), buf, C.c_size_t(len(buf))), "group_describe")
        return json.loads(buf.value.decode())

    def commitments(self, key: str, wtns: bytes | None):
        """groth16_commitments (incl. construct_r1cs) for this process's shard → (576-byte block, Timings).
        wtns=None re-uses the witness already resident on the device."""
        out = (C.c_uint8 * COMMITMENTS_BYTES)()
        tm = Timings()
        _pcheck(lib().groth16_commitments(self._h, key.encode(), wtns, C.c_size_t(len(wtns) if wtns else 0), out, C.byref(tm)), "commitments")
        return bytes(out), tm

    def assemble(self, key: str, wtns: bytes, points: bytes, r: int | None = None, s: int | None = None):
        pj, qj = C.create_string_buffer(1 << 14), C.create_string_buffer(1 << 20)
        rb, sb = _le32(r), _le32(s)
        _pcheck(lib().groth16_assemble_proof(self._h, key.encode(), wtns, C.c_size_t(len(wtns)), points, rb, sb,
                                             pj, C.c_size_t(len(pj)), qj, C.c_size_t(len(qj))), "assemble_proof")
        return pj.value.decode(), qj.value.decode()

    def _json_bufs(self):
        """the proof and public JSON buffers of prove_mem / prove_packed, made once"""
        if not hasattr(self, "_bufs"):
            self._bufs = (C.create_string_buffer(1 << 14), C.create_string_buffer(1 << 20))
        return self._bufs

    def prove_mem(self, key: str, wtns: bytes, r: int | None = None, s: int | None = None, resident: bool = False):
        """commitments + blinding + JSON in one call (the blinding terms are computed on a host thread while the GPU
        works).  resident=True re-uses the witness already uploaded by an earlier call."""
        pj, qj = self._json_bufs()
        rb, sb = _le32(r), _le32(s)
        tm = Timings()
        _pcheck(lib().groth16_prove_resident(self._h, key.encode(), wtns, C.c_size_t(len(wtns)), int(resident), rb, sb, pj,
                                             C.c_size_t(len(pj)), qj, C.c_size_t(len(qj)), C.byref(tm)), "prove_resident")
        return pj.value.decode(), qj.value.decode(), tm

    def prove_packed(self, key: str, wtnz: bytes, r: int | None = None, s: int | None = None):
        """groth16_prove_packed → (proof JSON, public JSON, Timings): prove_mem from a PACKED witness (wtns_pack), decoded on the
        GPU into the key's resident witness buffer; afterwards prove_mem(resident=True) proves the same witness.  A faulty packed
        witness raises ProverError (−2 "wtnz: element E: kind") and leaves no witness resident.  Single-device keys only (−3)."""
        pj, qj = self._json_bufs()
        rb, sb = _le32(r), _le32(s)
        tm = Timings()
        _pcheck(lib().groth16_prove_packed(self._h, key.encode(), _image(wtnz), C.c_size_t(len(wtnz)), rb, sb, pj, C.c_size_t(len(pj)), qj,
                                           C.c_size_t(len(qj)), C.byref(tm)), "prove_packed")
        return pj.value.decode(), qj.value.decode(), tm

    def prove_packed_files(self, witness: str, zkey: str, proof: str, public: str, device: str = "HIP"):
        """groth16_prove_packed_files: prove() with a packed witness file; a key the manager does not hold is loaded first"""
        _pcheck(lib().groth16_prove_packed_files(witness.encode(), zkey.encode(), proof.encode(), public.encode(), device.encode(), self._h), "prove_packed_files")

    # ---- distributed QAP front end (2, 4 or 8 strided shards): see include/groth16_prover.h ----
    def dist_supported(self, key: str) -> bool:
        return bool(lib().groth16_dist_supported(self._h, key.encode()))

    def dist_stage1(self, key: str, wtns: bytes | None):
        """→ (send ptr, recv ptr, rows, row_bytes, chunk_bytes): device buffers of exchange 1.  wtns=None: the witness is
        already resident (upload_witness_slice + all-gather + witness_ready)"""
        send, recv = C.c_void_p(), C.c_void_p()
        rows, rb, cb = C.c_uint32(), C.c_uint64(), C.c_uint64()
        _pcheck(lib().groth16_dist_stage1(self._h, key.encode(), wtns, C.c_size_t(len(wtns) if wtns else 0), C.byref(send), C.byref(recv), C.byref(rows), C.byref(rb), C.byref(cb)), "dist_stage1")
        return send.value, recv.value, rows.value, rb.value, cb.value

    def upload_witness_slice(self, key: str, wtns: bytes):
        """this rank's 1/shard_count of the witness → its place in the device witness buffer.
        → (device pointer of the whole buffer, bytes per rank of the in-place all-gather that completes it)"""
        ptr, sb = C.c_void_p(), C.c_uint64()
        _pcheck(lib().groth16_upload_witness_slice(self._h, key.encode(), wtns, C.c_size_t(len(wtns)), C.byref(ptr), C.byref(sb)), "upload_witness_slice")
        return ptr.value, sb.value

    def witness_ready(self, key: str):
        _pcheck(lib().groth16_witness_ready(self._h, key.encode()), "witness_ready")

    def dist_stage2(self, key: str):
        """→ (send ptr, recv ptr) of exchange 2 (same geometry as exchange 1)"""
        send, recv = C.c_void_p(), C.c_void_p()
        _pcheck(lib().groth16_dist_stage2(self._h, key.encode(), C.byref(send), C.byref(recv)), "dist_stage2")
        return send.value, recv.value

    def dist_exchange_done(self, key: str):
        """the caller confirms that exchange 2 delivered: the next commitments(key, None) finishes from those rows"""
        _pcheck(lib().groth16_dist_exchange_done(self._h, key.encode()), "dist_exchange_done")

    def prove_files(self, witness: str, zkey: str, proof: str, public: str, device: str = "HIP"):
        """groth16_prove — src/lib.rs:33-61: files in, files out (the reference's timed region)"""
        return self.prove(witness, zkey, proof, public, device)

    def last_timings(self, key: str) -> Timings:
        tm = Timings()
        _pcheck(lib().groth16_last_timings(self._h, key.encode(), C.byref(tm)), "last_timings")
        return tm

    def prove(self, witness: str, zkey: str, proof: str, public: str, device: str = "HIP"):
        """groth16_prove — src/lib.rs:33-61"""
        _pcheck(lib().groth16_prove(witness.encode(), zkey.encode(), proof.encode(), public.encode(), device.encode(), self._h), "groth16_prove")


PROVER_SYMBOLS = """
groth16_cache_manager_new groth16_cache_manager_free groth16_prove groth16_cache_load groth16_cache_load_file
groth16_cache_contains groth16_cache_evict groth16_commitments groth16_sum_commitments groth16_assemble_proof
groth16_prove_mem groth16_prove_resident groth16_cache_info groth16_last_error groth16_last_timings
groth16_dist_supported groth16_dist_stage1 groth16_dist_stage2 groth16_dist_exchange_done groth16_upload_witness_slice
groth16_witness_ready groth16_cache_load_devices groth16_parse_device groth16_cache_set_budget groth16_cache_info_sized
groth16_verify groth16_verify_json groth16_verify_last_error groth16_group_describe groth16_cache_tables_ready
groth16_cache_manager_prewarm groth16_verify_batch groth16_verify_batch_last_timings
groth16_verify_batch_combined groth16_verify_combined_coefficients
groth16_vkset_new groth16_vkset_info groth16_vkset_free groth16_verify_batch_mixed
groth16_zkey_check groth16_zkey_check_file
groth16_r1cs_info groth16_r1cs_load groth16_r1cs_load_file groth16_r1cs_get_info groth16_r1cs_free
groth16_witness_check groth16_witness_check_file groth16_r1cs_match_zkey
groth16_ptau_info groth16_zkey_verify_ptau groth16_zkey_verify_ptau_file
groth16_zkey_new_size groth16_zkey_new groth16_zkey_new_file
groth16_setup_toxic_check groth16_setup groth16_setup_file
groth16_zkey_contribute groth16_zkey_contribute_file groth16_zkey_contributions
groth16_ptau_prepared_size groth16_ptau_prepare groth16_ptau_prepare_file
groth16_ptau_new_size groth16_ptau_new groth16_ptau_new_file
groth16_ptau_contribute groth16_ptau_contribute_file groth16_ptau_contributions
groth16_beacon_digest groth16_ptau_beacon groth16_ptau_beacon_file groth16_zkey_beacon groth16_zkey_beacon_file
groth16_ptau_beacons groth16_zkey_beacons
groth16_ptau_verify groth16_ptau_verify_file
groth16_points_pack groth16_points_unpack groth16_ptau_packed_size groth16_ptau_unpacked_size
groth16_ptau_pack groth16_ptau_pack_file groth16_ptau_unpack groth16_ptau_unpack_file
groth16_ptau_truncated_size groth16_ptau_truncate groth16_ptau_truncate_file
groth16_wtns_packed_size groth16_wtns_pack groth16_wtns_pack_file groth16_wtns_unpack_host groth16_wtns_unpack_host_file
groth16_wtns_unpack groth16_wtns_unpack_file groth16_prove_packed groth16_prove_packed_files
groth16_witness_check_packed groth16_witness_check_packed_file
groth16_zkey_unpacked_size groth16_zkey_packed_bound groth16_zkey_pack groth16_zkey_pack_file groth16_zkey_unpack groth16_zkey_unpack_file
groth16_zkey_coefs_pack groth16_zkey_coefs_unpack groth16_cache_load_packed groth16_cache_load_packed_file groth16_prove_zkez_files
""".split()
# (the int / void / pointer-returning entry points of include/groth16_prover.h; groth16_zkey_export_vk returns int64_t)


def parse_device(device: str, cap: int = 64):
    """device string of groth16_prove → list of device ids ("HIP:0-7" → [0, …, 7]); raises ProverError for a bad string"""
    ids = (C.c_int * cap)()
    n = lib().groth16_parse_device(device.encode(), ids, cap)
    if n < 0:
        _pcheck(n, "parse_device")
    return [ids[i] for i in range(min(n, cap))]


def pairing(p_aff: np.ndarray, q_aff: np.ndarray) -> np.ndarray:
    """pairing — wrappers/rust/icicle-core/src/pairing/mod.rs:14-22.  Affine standard-form points in, the 12 Fq
    coefficients of e(P,Q) out (host computation, as in the reference)."""
    out = np.zeros((12, 4), dtype=np.uint64)
    check(lib().bn254_pairing(ptr_of(np.ascontiguousarray(p_aff)), ptr_of(np.ascontiguousarray(q_aff)), ptr_of(out)), "pairing")
    return out


def gt_op(op: str, a: np.ndarray, b=None) -> np.ndarray:
    """TargetField arithmetic (bn254_pairing_target_field_{add,sub,mul,inv,pow}); `b` is an int for pow."""
    out = np.zeros((12, 4), dtype=np.uint64)
    f = getattr(lib(), "bn254_pairing_target_field_" + op)
    a = np.ascontiguousarray(a)
    if op == "inv":
        f(ptr_of(a), ptr_of(out))
    elif op == "pow":
        f(ptr_of(a), C.c_int(int(b)), ptr_of(out))
    else:
        f(ptr_of(a), ptr_of(np.ascontiguousarray(b)), ptr_of(out))
    return out


def groth16_verify_json(proof_json: str, public_json: str, vk_json: str) -> bool:
    """groth16_verify_helper — src/proof_helper.rs:319-372 on JSON texts."""
    rc = lib().groth16_verify_json(proof_json.encode(), public_json.encode(), vk_json.encode())
    if rc < 0:
        _verify_fail(rc, "groth16_verify")
    return rc == 1


def pairing_batch(P: np.ndarray, Q: np.ndarray) -> np.ndarray:
    """e(P[i], Q[i]) for n pairs on the current device (icicle_snark_pairing_batch): P (n,2,4) / Q (n,4,4) standard-form
    affine u64, (0,0) = identity; returns (n,12,4) in bn254_pairing's basis and form."""
    P = np.ascontiguousarray(P, dtype=np.uint64).reshape(-1, 2, 4)
    Q = np.ascontiguousarray(Q, dtype=np.uint64).reshape(-1, 4, 4)
    n = len(P)
    if len(Q) != n:
        raise ValueError("pairing_batch: P and Q differ in length")
    out = np.zeros((n, 12, 4), dtype=np.uint64)
    if n == 0:
        return out
    dp, dq, do = DeviceVec.from_host(P), DeviceVec.from_host(Q), DeviceVec(out.nbytes)
    try:
        check(lib().icicle_snark_pairing_batch(ptr_of(dp), ptr_of(dq), C.c_uint64(n), None, ptr_of(do)), "pairing_batch")
        check(lib().icicle_device_synchronize(), "pairing_batch")
        out = do.to_host(out.shape)
    finally:
        for d in (dp, dq, do):
            d.free()
    return out


def groth16_verify_batch(proofs, publics, vk: str, device: str = "HIP") -> list:
    """verify n proofs (JSON texts) against one verification key on one GPU (groth16_verify_batch): one verdict per item,
    each what groth16_verify_json's C function returns for it — 1 accepted, 0 rejected, negative = that item's format
    error.  Raises ProverError for a malformed vk, a bad device string or a device failure."""
    n = len(proofs)
    if len(publics) != n:
        raise ValueError("groth16_verify_batch: proofs and publics differ in length")
    pa = (C.c_char_p * max(n, 1))(*[p.encode() if isinstance(p, str) else p for p in proofs])
    qa = (C.c_char_p * max(n, 1))(*[q.encode() if isinstance(q, str) else q for q in publics])
    out = (C.c_int32 * max(n, 1))()
    rc = lib().groth16_verify_batch(pa, qa, C.c_int(n), vk.encode(), device.encode(), out)
    if rc != 0:
        _verify_fail(rc, "groth16_verify_batch")
    return [int(out[i]) for i in range(n)]


def groth16_verify_batch_combined(proofs, publics, vk: str, device: str = "HIP", seed=None):
    """groth16_verify_batch's verdicts through one randomised pairing equation over the whole batch
    (groth16_verify_batch_combined): returns (verdicts, path) — path 1 when the combined equation accepted every live item, 0
    when the per-item stage decided.  `seed`: 32 secret bytes, or None for the operating system's randomness; a seed known to
    whoever made the proofs voids the 2^-127 bound on accepting an invalid item."""
    n = len(proofs)
    if len(publics) != n:
        raise ValueError("groth16_verify_batch_combined: proofs and publics differ in length")
    sd = _seed32(seed, "groth16_verify_batch_combined")
    pa = (C.c_char_p * max(n, 1))(*[p.encode() if isinstance(p, str) else p for p in proofs])
    qa = (C.c_char_p * max(n, 1))(*[q.encode() if isinstance(q, str) else q for q in publics])
    out = (C.c_int32 * max(n, 1))()
    path = C.c_int32(0)
    rc = lib().groth16_verify_batch_combined(pa, qa, C.c_int(n), vk.encode(), device.encode(), sd, out, C.byref(path))
    if rc != 0:
        _verify_fail(rc, "groth16_verify_batch_combined")
    return [int(out[i]) for i in range(n)], int(path.value)


class MixedReport(C.Structure):
    _fields_ = [("path", C.c_int32), ("keys_live", C.c_uint32), ("keys_fallback", C.c_uint32), ("parse_ms", C.c_double),
                ("device_ms", C.c_double)]


class VkSet:
    """a set of verification keys (JSON texts) checked once and kept on one device (groth16_vkset_new), for verify(): proofs of
    many keys, interleaved, in one call (groth16_verify_batch_mixed).  Raises ProverError for a refused key ("key <index>: …",
    before any device is touched), a bad device string or a device failure.  A context manager; free() releases the device
    memory, and a freed set refuses further calls."""

    def __init__(self, vks, device: str = "HIP"):
        self._h = None
        n = len(vks)
        arr = (C.c_char_p * max(n, 1))(*[v.encode() if isinstance(v, str) else v for v in vks])
        h = C.c_void_p()
        rc = lib().groth16_vkset_new(arr, C.c_int(n), device.encode(), C.byref(h))
        if rc != 0:
            _verify_fail(rc, "groth16_vkset_new")
        self._h = h

    def _handle(self):
        if self._h is None:
            raise ProverError("VkSet: the set has been freed")
        return self._h

    @property
    def n_keys(self) -> int:
        return int(lib().groth16_vkset_info(self._handle(), C.c_int(-1), None))

    def n_public(self, k: int) -> int:
        out = C.c_uint32(0)
        rc = lib().groth16_vkset_info(self._handle(), C.c_int(k), C.byref(out))
        if rc != 0:
            _verify_fail(rc, "groth16_vkset_info")
        return int(out.value)

    def verify(self, proofs, publics, key_of, seed=None):
        """(verdicts, report): verdicts[i] is groth16_verify_batch's verdict for item i under key key_of[i] (−2 for a key index
        outside the set); report.path is 1 when the one randomised equation accepted every live item, else 0 with
        report.keys_fallback keys sent through the per-item stage.  `seed`: 32 secret bytes, or None for the operating
        system's randomness — see groth16_verify_batch_combined."""
        n = len(proofs)
        if len(publics) != n or len(key_of) != n:
            raise ValueError("VkSet.verify: proofs, publics and key_of differ in length")
        sd = _seed32(seed, "VkSet.verify")
        pa = (C.c_char_p * max(n, 1))(*[p.encode() if isinstance(p, str) else p for p in proofs])
        qa = (C.c_char_p * max(n, 1))(*[q.encode() if isinstance(q, str) else q for q in publics])
        ka = (C.c_int32 * max(n, 1))(*[int(k) for k in key_of])
        out = (C.c_int32 * max(n, 1))()
        rep = MixedReport()
        rc = lib().groth16_verify_batch_mixed(self._handle(), pa, qa, ka, C.c_int(n), sd, out, C.byref(rep))
        if rc != 0:
            _verify_fail(rc, "groth16_verify_batch_mixed")
        return [int(out[i]) for i in range(n)], rep

    def free(self):
        if self._h is not None:
            lib().groth16_vkset_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def verify_combined_coefficients(seed: bytes, first: int, count: int) -> list:
    """the combined verifier's coefficients z_first … z_{first+count−1} for a 32-byte seed, as integers (no GPU)"""
    sd = _seed32(bytes(seed), "verify_combined_coefficients")   # not optional here
    out = (C.c_uint8 * (16 * max(count, 1)))()
    lib().groth16_verify_combined_coefficients(sd, C.c_uint64(first), C.c_uint64(count), out)
    raw = bytes(out)
    return [int.from_bytes(raw[16 * k:16 * k + 16], "little") for k in range(count)]


def pairing_product(P: np.ndarray, Q: np.ndarray) -> np.ndarray:
    """Π e(P[i], Q[i]) on the current device (icicle_snark_pairing_product): P (n,2,4) / Q (n,4,4) as pairing_batch takes them;
    returns one (12,4) value in bn254_pairing's basis and form (1 for n = 0)."""
    P = np.ascontiguousarray(P, dtype=np.uint64).reshape(-1, 2, 4)
    Q = np.ascontiguousarray(Q, dtype=np.uint64).reshape(-1, 4, 4)
    n = len(P)
    if len(Q) != n:
        raise ValueError("pairing_product: P and Q differ in length")
    out = np.zeros((12, 4), dtype=np.uint64)
    bufs = [DeviceVec(out.nbytes)]
    if n:
        bufs += [DeviceVec.from_host(P), DeviceVec.from_host(Q)]
    try:
        check(lib().icicle_snark_pairing_product(ptr_of(bufs[1]) if n else None, ptr_of(bufs[2]) if n else None, C.c_uint64(n), None,
                                                 ptr_of(bufs[0])), "pairing_product")
        check(lib().icicle_device_synchronize(), "pairing_product")
        out = bufs[0].to_host(out.shape)
    finally:
        for d in bufs:
            d.free()
    return out


def msm_segmented(points: np.ndarray, scalars: np.ndarray, offsets, bits, cut: int = 0) -> np.ndarray:
    """out[s] = Σ scalars[k]·points[k] over offsets[s] ≤ k < offsets[s+1] on the current device (icicle_snark_msm_segmented):
    points (n,2,4) standard-form affine u64, (0,0) = identity; scalars (n,4); bits[s] ∈ {128, 254} = the bits walked in segment
    s; cut = entries per workgroup (0 = the default).  Returns (segments,2,4) canonical affine, (0,0) = identity."""
    points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 2, 4)
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    bits = np.ascontiguousarray(bits, dtype=np.uint8)
    ns = len(bits)
    if len(offsets) != ns + 1 or len(points) != len(scalars) or (ns and int(offsets[-1]) > len(points)):
        raise ValueError("msm_segmented: offsets, bits, points and scalars do not fit together")
    out = np.zeros((ns, 2, 4), dtype=np.uint64)
    if ns == 0:
        return out
    bufs = [DeviceVec(out.nbytes), DeviceVec.from_host(points), DeviceVec.from_host(scalars)]
    try:
        check(lib().icicle_snark_msm_segmented(ptr_of(bufs[1]), ptr_of(bufs[2]), ptr_of(offsets), C.c_uint32(ns), ptr_of(bits),
                                               C.c_uint32(cut), None, ptr_of(bufs[0])), "msm_segmented")
        check(lib().icicle_device_synchronize(), "msm_segmented")
        out = bufs[0].to_host(out.shape)
    finally:
        for d in bufs:
            d.free()
    return out


def groth16_verify_batch_last_timings():
    """(host parse ms, device ms) of this thread's last groth16_verify_batch"""
    a, b = C.c_double(), C.c_double()
    lib().groth16_verify_batch_last_timings(C.byref(a), C.byref(b))
    return a.value, b.value


def groth16_verify(proof: str, public: str, vk: str):
    """groth16_verify — src/lib.rs:63-82 (paths in; raises on a rejected proof like the reference's assert)."""
    rc = lib().groth16_verify(proof.encode(), public.encode(), vk.encode())
    if rc != 0:
        _verify_fail(rc, "groth16_verify")


class ZkeyReport(C.Structure):
    """Groth16ZkeyReport (include/groth16_prover.h): kind / section / index of the first fault, faults[s] per zkey section"""
    _fields_ = [("kind", C.c_int32), ("section", C.c_int32), ("index", C.c_uint64), ("faults", C.c_uint64 * 10),
                ("upload_ms", C.c_double), ("device_ms", C.c_double), ("pairing_ms", C.c_double)]


class ZkeyCheckOptions(C.Structure):
    _fields_ = [("slice_points", C.c_uint32), ("seed32", C.c_char_p)]


ZKEY_NONCANONICAL, ZKEY_OFF_CURVE, ZKEY_OFF_SUBGROUP, ZKEY_IDENTITY, ZKEY_PAIR_MISMATCH, ZKEY_COEFFICIENT = range(1, 7)


def _zkey_check(call, what, device, slice_points, seed):
    sd = _seed32(seed, what)
    opt = ZkeyCheckOptions(int(slice_points), C.cast(sd, C.c_char_p) if sd is not None else None)
    rep = ZkeyReport()
    rc = call(device.encode(), C.byref(opt), C.byref(rep))
    if rc not in (0, 1):
        _pcheck(rc, what)
    return rc == 1, rep


def zkey_check(zkey: bytes, device: str = "HIP", slice_points: int = 0, seed=None):
    """groth16_zkey_check: every point of the key on its curve (B2: in the subgroup), the coefficient records in range, the
    header pairs and B1 against B2 consistent.  Returns (ok, ZkeyReport); raises ProverError for a malformed file or a device
    error.  seed: 32 bytes for a reproducible test — leave it None otherwise (a secret, fresh seed is drawn)."""
    p = _image(zkey)
    return _zkey_check(lambda d, o, r: lib().groth16_zkey_check(p, C.c_size_t(len(zkey)), d, o, r), "zkey_check", device, slice_points, seed)


def zkey_check_file(path: str, device: str = "HIP", slice_points: int = 0, seed=None):
    """groth16_zkey_check_file: zkey_check on a mapped file"""
    return _zkey_check(lambda d, o, r: lib().groth16_zkey_check_file(os.fsencode(path), d, o, r), "zkey_check_file", device, slice_points, seed)


def zkey_export_vk(zkey: bytes) -> str:
    """groth16_zkey_export_vk: the key's verification_key.json text (host only: needs no GPU)"""
    f = lib().groth16_zkey_export_vk
    need = f(C.c_char_p(bytes(zkey)), C.c_size_t(len(zkey)), None, C.c_size_t(0))
    if need < 0:
        _pcheck(int(need), "zkey_export_vk")
    buf = C.create_string_buffer(need)
    f(C.c_char_p(bytes(zkey)), C.c_size_t(len(zkey)), buf, C.c_size_t(need))
    return buf.value.decode()


class R1csInfo(C.Structure):
    """Groth16R1csInfo (include/groth16_prover.h)"""
    _fields_ = [("n_wires", C.c_uint32), ("n_public", C.c_uint32), ("n_constraints", C.c_uint32), ("n_terms", C.c_uint64),
                ("device_bytes", C.c_uint64), ("walk_ms", C.c_double), ("upload_ms", C.c_double), ("device_ms", C.c_double)]


class WitnessReport(C.Structure):
    """Groth16WitnessReport: kind / index of the first fault, the counts"""
    _fields_ = [("kind", C.c_int32), ("index", C.c_uint64), ("noncanonical", C.c_uint64), ("failed", C.c_uint64),
                ("upload_ms", C.c_double), ("device_ms", C.c_double)]


class MatchReport(C.Structure):
    """Groth16R1csMatchReport: kind / index of the first fault, the differing rows of A and of B"""
    _fields_ = [("kind", C.c_int32), ("index", C.c_uint64), ("rows_a", C.c_uint64), ("rows_b", C.c_uint64), ("device_ms", C.c_double)]


WTNS_NONCANONICAL, WTNS_ONE, WTNS_CONSTRAINT = 1, 2, 3
MATCH_SIZES, MATCH_ROW_A, MATCH_ROW_B = 1, 2, 3


class PtauInfo(C.Structure):
    """Groth16PtauInfo: power, ceremonyPower, payload bytes per section id (0 = absent)"""
    _fields_ = [("power", C.c_uint32), ("ceremony_power", C.c_uint32), ("section_bytes", C.c_uint64 * 16)]


class VerifyReport(C.Structure):
    """Groth16ZkeyVerifyReport: kind (/ index for SIZES and HEADER) of the first fault, failed_mask with bit (kind − VERIFY_HEADER)
    per failing equation, `key` the embedded groth16_zkey_check report"""
    _fields_ = [("kind", C.c_int32), ("index", C.c_uint64), ("failed_mask", C.c_uint32), ("key", ZkeyReport),
                ("upload_ms", C.c_double), ("device_ms", C.c_double), ("pairing_ms", C.c_double)]


VERIFY_SIZES, VERIFY_KEY, VERIFY_HEADER, VERIFY_A, VERIFY_B1, VERIFY_B2, VERIFY_IC, VERIFY_C, VERIFY_H = range(1, 10)
VERIFY_KIND_NAMES = ["ok", "SIZES", "KEY", "HEADER", "A", "B1", "B2", "IC", "C", "H"]


class ZkeyNewOptions(C.Structure):
    _fields_ = [("heavy_column_terms", C.c_uint32)]


class ZkeyNewReport(C.Structure):
    """Groth16ZkeyNewReport: the key's sizes, the longest column, the heavy columns and their items, the stage times"""
    _fields_ = [("n_vars", C.c_uint32), ("n_public", C.c_uint32), ("domain", C.c_uint32), ("n_coeffs", C.c_uint64), ("zkey_bytes", C.c_uint64),
                ("longest_column", C.c_uint32), ("heavy_columns", C.c_uint32), ("heavy_items", C.c_uint32),
                ("upload_ms", C.c_double), ("device_ms", C.c_double), ("download_ms", C.c_double), ("write_ms", C.c_double)]


class SetupOptions(C.Structure):
    _fields_ = [("heavy_column_terms", C.c_uint32)]


class SetupReport(C.Structure):
    """Groth16SetupReport: ZkeyNewReport's fields, then the device time by stage"""
    _fields_ = ZkeyNewReport._fields_ + [("lagrange_ms", C.c_double), ("columns_ms", C.c_double), ("g1_ms", C.c_double), ("g2_ms", C.c_double)]


TOXIC_RANGE, TOXIC_ZERO, TOXIC_DOMAIN = 1, 2, 3
R_ORDER = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def toxic160(toxic):
    """(τ, α, β, γ, δ) as ints → the 160 bytes groth16_setup takes (any value below 2^256 is representable: the library judges it)"""
    toxic = tuple(toxic)
    if len(toxic) != 5:
        raise ValueError("toxic waste is (tau, alpha, beta, gamma, delta)")
    return (C.c_uint8 * 160).from_buffer_copy(b"".join(int(x).to_bytes(32, "little") for x in toxic))


def setup_toxic_check(toxic, domain_power: int) -> int:
    """groth16_setup_toxic_check → 0, or TOXIC_RANGE / TOXIC_ZERO / TOXIC_DOMAIN; host only"""
    rc = lib().groth16_setup_toxic_check(toxic160(toxic), C.c_uint32(domain_power))
    if rc < 0:
        _pcheck(rc, "setup_toxic_check")
    return rc


def r1cs_info(r1cs: bytes) -> R1csInfo:
    """groth16_r1cs_info: the counts of an .r1cs after the host walk that bounds every record (host only: needs no GPU)"""
    info = R1csInfo()
    _pcheck(lib().groth16_r1cs_info(_image(r1cs), C.c_size_t(len(r1cs)), C.byref(info)), "r1cs_info")
    return info


def zkey_new_size(r1cs: bytes):
    """groth16_zkey_new_size → (bytes of the key R1cs.new_zkey writes for this circuit, section 4's record count); host only"""
    size, coeffs = C.c_uint64(), C.c_uint64()
    _pcheck(lib().groth16_zkey_new_size(_image(r1cs), C.c_size_t(len(r1cs)), C.byref(size), C.byref(coeffs)), "zkey_new_size")
    return size.value, coeffs.value


def ptau_info(ptau, domain_power: int = -1) -> PtauInfo:
    """groth16_ptau_info: power and sections of a prepared .ptau (bytes, or a path that is mapped; host only: needs no GPU).
    domain_power >= 0 also asks whether the file serves a key of that domain (ProverError −3 / −2 when not)."""
    info = PtauInfo()
    if _is_path(ptau):
        import mmap
        with open(ptau, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
            view = np.frombuffer(mm, dtype=np.uint8)
            try:
                _pcheck(lib().groth16_ptau_info(_image(view), C.c_size_t(len(view)), C.c_int32(domain_power), C.byref(info)), "ptau_info")
            finally:
                del view
        return info
    _pcheck(lib().groth16_ptau_info(_image(ptau), C.c_size_t(len(ptau)), C.c_int32(domain_power), C.byref(info)), "ptau_info")
    return info


class R1cs:
    """An .r1cs (bytes, or a path that is mapped) kept on one GPU: groth16_r1cs_load / groth16_witness_check."""

    def __init__(self, r1cs, device: str = "HIP"):
        self._h = C.c_void_p()
        if _is_path(r1cs):
            _pcheck(lib().groth16_r1cs_load_file(os.fsencode(r1cs), device.encode(), C.byref(self._h)), "r1cs_load_file")
        else:
            _pcheck(lib().groth16_r1cs_load(_image(r1cs), C.c_size_t(len(r1cs)), device.encode(), C.byref(self._h)), "r1cs_load")
        self.info = R1csInfo()
        _pcheck(lib().groth16_r1cs_get_info(self._h, C.byref(self.info)), "r1cs_get_info")

    def _verdict(self, rc, rep, what):
        if rc not in (0, 1):
            _pcheck(rc, what)
        return rc == 1, rep

    def check(self, wtns):
        """groth16_witness_check → (ok, WitnessReport); wtns: the .wtns image, or a path.  Raises ProverError for a malformed
        file, a witness of another size or a device error."""
        rep = WitnessReport()
        if _is_path(wtns):
            return self._verdict(lib().groth16_witness_check_file(self._h, os.fsencode(wtns), C.byref(rep)), rep, "witness_check_file")
        return self._verdict(lib().groth16_witness_check(self._h, _image(wtns), C.c_size_t(len(wtns)), C.byref(rep)), rep, "witness_check")

    def check_packed(self, wtnz):
        """groth16_witness_check_packed → (ok, WitnessReport): check() of a PACKED witness (wtns_pack; the image, or a path), decoded
        on the GPU.  A faulty packed witness raises ProverError (−2 "wtnz: element E: kind")."""
        rep = WitnessReport()
        if _is_path(wtnz):
            return self._verdict(lib().groth16_witness_check_packed_file(self._h, os.fsencode(wtnz), C.byref(rep)), rep, "witness_check_packed_file")
        return self._verdict(lib().groth16_witness_check_packed(self._h, _image(wtnz), C.c_size_t(len(wtnz)), C.byref(rep)), rep, "witness_check_packed")

    def match_zkey(self, zkey, seed=None):
        """groth16_r1cs_match_zkey → (ok, MatchReport): the key's section 4 against this circuit's A and B.  seed: 32 bytes for a
        reproducible test — leave it None otherwise (a secret, fresh seed is drawn)."""
        sd = _seed32(seed, "match_zkey")
        rep = MatchReport()
        return self._verdict(lib().groth16_r1cs_match_zkey(self._h, _image(zkey), C.c_size_t(len(zkey)), sd, C.byref(rep)), rep, "r1cs_match_zkey")

    def verify_zkey(self, zkey, ptau, seed=None):
        """groth16_zkey_verify_ptau → (ok, VerifyReport): is the key this circuit's Groth16 key over this prepared .ptau?  zkey
        and ptau: both images, or both paths (mapped; only the ptau ranges that are read are touched).  seed: 32 bytes for a
        reproducible test — leave it None otherwise (a secret, fresh seed is drawn)."""
        sd = _seed32(seed, "verify_zkey")
        rep = VerifyReport()
        paths = [_is_path(x) for x in (zkey, ptau)]
        if all(paths):
            return self._verdict(lib().groth16_zkey_verify_ptau_file(self._h, os.fsencode(zkey), os.fsencode(ptau), sd, C.byref(rep)), rep, "zkey_verify_ptau_file")
        if any(paths):
            raise TypeError("verify_zkey: zkey and ptau are both images or both paths")
        return self._verdict(lib().groth16_zkey_verify_ptau(self._h, _image(zkey), C.c_size_t(len(zkey)), _image(ptau), C.c_size_t(len(ptau)), sd, C.byref(rep)),
                             rep, "zkey_verify_ptau")

    def new_zkey(self, ptau, out=None, heavy_column_terms: int = 0):
        """groth16_zkey_new → (zkey bytes | None, ZkeyNewReport): this circuit's proving key over the prepared .ptau, before any
        phase-2 contribution (gamma = delta = 1: NOT a key to prove with in production).  ptau: the image, and the key comes back
        as bytes; or a path together with `out`, the path the key is written to (None comes back).  heavy_column_terms: 0 = the
        default.  Raises ProverError (−2 an unprepared ptau or a ptau point failing its lane test, −3 a ptau of too low a power)."""
        opt, rep = ZkeyNewOptions(int(heavy_column_terms)), ZkeyNewReport()
        if _path_or_image("new_zkey", ptau, out):
            _pcheck(lib().groth16_zkey_new_file(self._h, os.fsencode(ptau), os.fsencode(out), C.byref(opt), C.byref(rep)), "zkey_new_file")
            return None, rep
        buf = _sized_twice(lambda buf, room: lib().groth16_zkey_new(self._h, _image(ptau), C.c_size_t(len(ptau)), buf, room, C.byref(opt), C.byref(rep)),
                           rep, "zkey_bytes", "zkey_new")
        return buf.raw, rep

    def setup(self, out=None, toxic=None, heavy_column_terms: int = 0):
        """groth16_setup → (zkey bytes | None, SetupReport): this circuit's proving key made directly from toxic waste, no .ptau.
        WHOEVER RAN THIS CALL CAN FORGE PROOFS FOR THE KEY: for development, CI, benchmarks and single-party deployments.  toxic:
        (τ, α, β, γ, δ) as ints, for tests and reproducible benchmarks; None = the operating system's randomness.  out: a path the
        key is written to (None comes back); None: the key comes back as bytes.  Raises ProverError (−2 faulty toxic waste)."""
        opt, rep = SetupOptions(int(heavy_column_terms)), SetupReport()
        tx = toxic160(toxic) if toxic is not None else None
        if out is not None:
            _pcheck(lib().groth16_setup_file(self._h, tx, os.fsencode(out), C.byref(opt), C.byref(rep)), "setup_file")
            return None, rep
        buf = _sized_twice(lambda buf, room: lib().groth16_setup(self._h, tx, buf, room, C.byref(opt), C.byref(rep)), rep, "zkey_bytes", "setup")
        return buf.raw, rep

    def close(self):
        if self._h:
            lib().groth16_r1cs_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ZkeyContributeOptions(C.Structure):
    _fields_ = [("fixed_delta", C.POINTER(C.c_uint8))]


class ZkeyContributeReport(C.Structure):
    """Groth16ZkeyContributeReport: the record's number, the points of sections 8 and 9, the output's size, the first faulty
    point (section, kind, index) and how many there are, the stage times"""
    _fields_ = [("contribution", C.c_uint32), ("points_c", C.c_uint64), ("points_h", C.c_uint64), ("zkey_bytes", C.c_uint64),
                ("fault_section", C.c_int32), ("fault_kind", C.c_int32), ("fault_index", C.c_uint64), ("faults", C.c_uint64),
                ("upload_ms", C.c_double), ("device_ms", C.c_double), ("download_ms", C.c_double), ("write_ms", C.c_double)]


class ContributionsReport(C.Structure):
    """Groth16ContributionsReport: the record count, kind and index (records count from 1) of the first fault; .records: the
    (after1 bytes, name bytes) of the records whose bounds hold"""
    _fields_ = [("count", C.c_uint32), ("kind", C.c_int32), ("index", C.c_uint32)]
    records = ()
    beacons = {}


class ContributionInfo(C.Structure):
    _fields_ = [("after1", C.c_uint8 * 64), ("name", C.c_char * 256)]


CONTRIB_SECTION, CONTRIB_POINT, CONTRIB_POK, CONTRIB_HEADER, CONTRIB_PAIR, CONTRIB_BEACON = range(1, 7)
CONTRIB_KIND_NAMES = ["ok", "SECTION", "POINT", "POK", "HEADER", "PAIR", "BEACON"]
BEACON_ITER_EXP_MAX = 24


class BeaconInfo(C.Structure):
    """Groth16BeaconInfo: a beacon record's number (from 1), its beacon_hash and iter_exp as the record holds them"""
    _fields_ = [("index", C.c_uint32), ("hash", C.c_uint8 * 32), ("iter_exp", C.c_uint32)]


def _beacons(entry, image, cap):
    """groth16_ptau_beacons / groth16_zkey_beacons → {record number: (beacon_hash, iter_exp)} of the flagged records among
    those .records lists (the first `cap` of them): every key is the number of an entry of .records; host only"""
    infos = (BeaconInfo * cap)()
    n = getattr(lib(), entry)(_image(image), C.c_size_t(len(image)), infos, C.c_size_t(cap))
    if n < 0:
        _pcheck(n, entry)
    return {int(infos[i].index): (bytes(infos[i].hash), int(infos[i].iter_exp)) for i in range(min(n, cap))}


def beacon_digest(hash, iter_exp: int) -> bytes:
    """groth16_beacon_digest: beacon_hash (32 bytes) hashed 2^iter_exp times in sequence with SHA-256 — the public "secret" of a
    beacon; host only.  Raises ProverError −3 for iter_exp above 24."""
    h = _seed32(hash, "beacon_digest", "hash")
    if h is None:
        raise ValueError("beacon_digest: hash must be 32 bytes")
    out = (C.c_uint8 * 32)()
    _pcheck(lib().groth16_beacon_digest(h, C.c_uint32(iter_exp), out), "beacon_digest")
    return bytes(out)


def _beacon(tool, report_type, size_field, image, beacon_hash, iter_exp, name, out, device):
    """groth16_ptau_beacon / groth16_zkey_beacon and their _file entries: contribute's calling convention with the beacon's
    parameters in the secret's place"""
    h = _seed32(beacon_hash, tool, "beacon_hash")
    if h is None:
        raise ValueError(f"{tool}: beacon_hash must be 32 bytes")
    rep = report_type()
    nm = name.encode() if isinstance(name, str) else bytes(name)
    if _path_or_image(tool, image, out):
        _pcheck(getattr(lib(), f"groth16_{tool}_file")(os.fsencode(image), os.fsencode(out), h, C.c_uint32(iter_exp), nm, device.encode(), C.byref(rep)), f"{tool}_file")
        return None, rep
    entry = getattr(lib(), f"groth16_{tool}")
    buf = _sized_twice(lambda buf, room: entry(_image(image), C.c_size_t(len(image)), h, C.c_uint32(iter_exp), nm, buf, room, device.encode(), C.byref(rep)),
                       rep, size_field, tool)
    return buf.raw, rep


def zkey_beacon(zkey, beacon_hash, iter_exp: int, name="", out=None, device: str = "HIP"):
    """groth16_zkey_beacon → (zkey bytes | None, ZkeyContributeReport): the random beacon of phase 2 — zkey_contribute with the
    secret beacon_digest(beacon_hash, iter_exp), which anybody can recompute, and a record that says so (bit 31 of its name_len,
    beacon_hash and iter_exp behind the name); zkey_contributions audits it (CONTRIB_BEACON) and lists it (.beacons).  zkey, out,
    name, device as zkey_contribute's.  Raises ProverError (−3 iter_exp above 24; else as zkey_contribute)."""
    return _beacon("zkey_beacon", ZkeyContributeReport, "zkey_bytes", zkey, beacon_hash, iter_exp, name, out, device)


def zkey_contribute(zkey, secret=None, name="", out=None, device: str = "HIP", delta=None):
    """groth16_zkey_contribute → (zkey bytes | None, ZkeyContributeReport): one phase-2 contribution applied on the GPU — the
    header's delta times delta', sections 8 and 9 times its inverse, one record appended to section 10 (this library's own
    layout: include/groth16_prover.h).  zkey: the image, and the new key comes back as bytes; or a path together with `out`, the
    path the new key is written to (None comes back).  secret: 32 bytes, None draws from the operating system.  name: str or bytes,
    at most 255 bytes.  delta: delta' itself as an integer in [1, r), for tests and reproducible runs.  Raises ProverError (−2 a
    faulty point of section 8 or 9 or a malformed section 10, −3 a name too long or a bad delta)."""
    sd = _seed32(secret, "zkey_contribute", "secret")
    fd = _seed32(_le32(delta), "zkey_contribute")
    opt, rep = ZkeyContributeOptions(C.cast(fd, C.POINTER(C.c_uint8)) if fd is not None else None), ZkeyContributeReport()
    nm = name.encode() if isinstance(name, str) else bytes(name)
    if _path_or_image("zkey_contribute", zkey, out):
        _pcheck(lib().groth16_zkey_contribute_file(os.fsencode(zkey), os.fsencode(out), sd, nm, device.encode(), C.byref(opt), C.byref(rep)), "zkey_contribute_file")
        return None, rep
    buf = _sized_twice(lambda buf, room: lib().groth16_zkey_contribute(_image(zkey), C.c_size_t(len(zkey)), sd, nm, buf, room, device.encode(), C.byref(opt), C.byref(rep)),
                       rep, "zkey_bytes", "zkey_contribute")
    return buf.raw, rep


def zkey_contributions(zkey):
    """groth16_zkey_contributions → (ok, ContributionsReport with .records): is section 10 a chain of valid contributions from
    delta = 1 to the header's delta1, and do delta1 and delta2 pair?  Host only: needs no GPU.  It does NOT show that sections 8
    and 9 follow delta2: that is R1cs.verify_zkey's."""
    rep = ContributionsReport()
    cap = min(len(zkey) // 164 + 1, 4096)   # a record is at least 164 bytes; .records holds the first 4096
    infos = (ContributionInfo * cap)()
    rc = lib().groth16_zkey_contributions(_image(zkey), C.c_size_t(len(zkey)), C.byref(rep), infos, C.c_size_t(cap))
    if rc not in (0, 1):
        _pcheck(rc, "zkey_contributions")
    held = rep.count if rep.kind != CONTRIB_SECTION else max(int(rep.index) - 1, 0)
    rep.records = [(bytes(infos[i].after1), infos[i].name) for i in range(min(held, cap))]
    rep.beacons = _beacons("groth16_zkey_beacons", zkey, cap)
    return rc == 1, rep


class PtauPrepareReport(C.Structure):
    """Groth16PtauPrepareReport: the power, the points of sections 12 to 15, the output's size, the first faulty point (section,
    kind, element), the stage times"""
    _fields_ = [("power", C.c_uint32), ("points", C.c_uint64 * 4), ("ptau_bytes", C.c_uint64),
                ("fault_section", C.c_int32), ("fault_kind", C.c_int32), ("fault_index", C.c_uint64),
                ("upload_ms", C.c_double), ("device_ms", C.c_double), ("download_ms", C.c_double), ("write_ms", C.c_double)]


def ptau_prepared_size(ptau: bytes) -> int:
    """groth16_ptau_prepared_size: the bytes of the file ptau_prepare writes for this UNPREPARED .ptau; host only.  Raises
    ProverError −2 for a malformed file, with a text of its own for one that is already prepared."""
    size = C.c_uint64()
    _pcheck(lib().groth16_ptau_prepared_size(_image(ptau), C.c_size_t(len(ptau)), C.byref(size)), "ptau_prepared_size")
    return size.value


def ptau_prepare(ptau, out=None, device: str = "HIP"):
    """groth16_ptau_prepare → (ptau bytes | None, PtauPrepareReport): sections 12 to 15 made on the GPU from sections 2 to 5 of an
    unprepared powers-of-tau file, what `snarkjs powersoftau prepare phase2` makes (include/groth16_prover.h has the definition,
    and what section 12's last block is).  ptau: the image, and the prepared file comes back as bytes; or a path together with
    `out`, the path the prepared file is written to (None comes back).  Raises ProverError (−2 a malformed or already prepared
    file, or a faulty point: section, element and kind in the text)."""
    rep = PtauPrepareReport()
    if _path_or_image("ptau_prepare", ptau, out):
        rc = lib().groth16_ptau_prepare_file(os.fsencode(ptau), os.fsencode(out), device.encode(), C.byref(rep))
        if rc != 1:
            _pcheck(rc, "ptau_prepare_file")
        return None, rep
    size = ptau_prepared_size(ptau)
    buf, got = C.create_string_buffer(size), C.c_uint64()
    rc = lib().groth16_ptau_prepare(_image(ptau), C.c_size_t(len(ptau)), buf, C.c_size_t(size), C.byref(got), device.encode(), C.byref(rep))
    if rc != 1:
        _pcheck(rc, "ptau_prepare")
    return buf.raw[:got.value], rep


class PtauContributeOptions(C.Structure):
    _fields_ = [("fixed_tau", C.POINTER(C.c_uint8)), ("fixed_alpha", C.POINTER(C.c_uint8)), ("fixed_beta", C.POINTER(C.c_uint8))]


class PtauContributeReport(C.Structure):
    """Groth16PtauContributeReport: the record's number, the power, the points of sections 2 to 5, the output's size, the first
    faulty point (section, kind, element), the stage times"""
    _fields_ = [("contribution", C.c_uint32), ("power", C.c_uint32), ("points", C.c_uint64 * 4), ("ptau_bytes", C.c_uint64),
                ("fault_section", C.c_int32), ("fault_kind", C.c_int32), ("fault_index", C.c_uint64),
                ("upload_ms", C.c_double), ("device_ms", C.c_double), ("download_ms", C.c_double), ("write_ms", C.c_double)]


class PtauContributionsReport(C.Structure):
    """Groth16PtauContributionsReport: the record count, kind (CONTRIB_*) and index (records count from 1) of the first fault;
    .records: (tau1, alpha1, beta1, tau2, beta2, name) bytes of the records whose bounds hold"""
    _fields_ = [("count", C.c_uint32), ("kind", C.c_int32), ("index", C.c_uint32)]
    records = ()
    beacons = {}


class PtauContributionInfo(C.Structure):
    _fields_ = [("tau1", C.c_uint8 * 64), ("alpha1", C.c_uint8 * 64), ("beta1", C.c_uint8 * 64), ("tau2", C.c_uint8 * 128), ("beta2", C.c_uint8 * 128),
                ("name", C.c_char * 256)]


def ptau_new_size(power: int) -> int:
    """groth16_ptau_new_size: the bytes of ptau_new's file; host only.  Raises ProverError −3 for a power above 27."""
    size = C.c_uint64()
    _pcheck(lib().groth16_ptau_new_size(C.c_uint32(power), C.byref(size)), "ptau_new_size")
    return size.value


def ptau_new(power: int, out=None):
    """groth16_ptau_new → bytes | None: the starting file of a powers-of-tau ceremony, tau = alpha = beta = 1 (every point a
    generator, section 7 with no record).  Host only: needs no GPU.  out: a path to write the file to (None comes back)."""
    if out is not None:
        _pcheck(lib().groth16_ptau_new_file(C.c_uint32(power), os.fsencode(out)), "ptau_new_file")
        return None
    size = ptau_new_size(power)
    buf, got = C.create_string_buffer(size), C.c_uint64()
    _pcheck(lib().groth16_ptau_new(C.c_uint32(power), buf, C.c_size_t(size), C.byref(got)), "ptau_new")
    return buf.raw[:got.value]


def ptau_contribute(ptau, secret=None, name="", out=None, device: str = "HIP", tau=None, alpha=None, beta=None):
    """groth16_ptau_contribute → (ptau bytes | None, PtauContributeReport): one participant's secrets applied on the GPU to every
    point of sections 2 to 6 of an UNPREPARED powers-of-tau file, one record appended to section 7 (this library's own layout:
    include/groth16_prover.h).  ptau: the image, and the new file comes back as bytes; or a path together with `out`, the path the
    new file is written to (None comes back).  secret: 32 bytes, None draws from the operating system.  name: str or bytes, at
    most 255 bytes.  tau, alpha, beta: the secrets themselves as integers in [1, r), for tests and reproducible runs.  Raises
    ProverError (−2 a faulty point, a prepared file, a malformed or stale section 7; −3 a name too long or a bad fixed secret)."""
    sd = _seed32(secret, "ptau_contribute", "secret")
    fixed = [_seed32(_le32(v), "ptau_contribute") for v in (tau, alpha, beta)]
    opt = PtauContributeOptions(*[C.cast(f, C.POINTER(C.c_uint8)) if f is not None else None for f in fixed])
    rep = PtauContributeReport()
    nm = name.encode() if isinstance(name, str) else bytes(name)
    if _path_or_image("ptau_contribute", ptau, out):
        _pcheck(lib().groth16_ptau_contribute_file(os.fsencode(ptau), os.fsencode(out), sd, nm, device.encode(), C.byref(opt), C.byref(rep)), "ptau_contribute_file")
        return None, rep
    buf = _sized_twice(lambda buf, room: lib().groth16_ptau_contribute(_image(ptau), C.c_size_t(len(ptau)), sd, nm, buf, room, device.encode(), C.byref(opt), C.byref(rep)),
                       rep, "ptau_bytes", "ptau_contribute")
    return buf.raw, rep


def ptau_beacon(ptau, beacon_hash, iter_exp: int, name="", out=None, device: str = "HIP"):
    """groth16_ptau_beacon → (ptau bytes | None, PtauContributeReport): the random beacon of phase 1 — ptau_contribute with the
    secret beacon_digest(beacon_hash, iter_exp), which anybody can recompute, and a record that says so (bit 31 of its name_len,
    beacon_hash and iter_exp behind the name); ptau_contributions audits it (CONTRIB_BEACON) and lists it (.beacons).  ptau, out,
    name, device as ptau_contribute's.  Raises ProverError (−3 iter_exp above 24; else as ptau_contribute)."""
    return _beacon("ptau_beacon", PtauContributeReport, "ptau_bytes", ptau, beacon_hash, iter_exp, name, out, device)


def ptau_contributions(ptau):
    """groth16_ptau_contributions → (ok, PtauContributionsReport with .records): is section 7 a chain of valid contributions from
    the generators to what sections 2 to 6 hold at their first elements, and do the G1 and G2 sides pair?  Host only: needs no
    GPU.  It does NOT show that the other powers of the file follow."""
    rep = PtauContributionsReport()
    cap = min(len(ptau) // 740 + 1, 4096)   # a record is at least 740 bytes; .records holds the first 4096
    infos = (PtauContributionInfo * cap)()
    rc = lib().groth16_ptau_contributions(_image(ptau), C.c_size_t(len(ptau)), C.byref(rep), infos, C.c_size_t(cap))
    if rc not in (0, 1):
        _pcheck(rc, "ptau_contributions")
    held = rep.count if rep.kind != CONTRIB_SECTION else max(int(rep.index) - 1, 0)
    rep.records = [(bytes(infos[i].tau1), bytes(infos[i].alpha1), bytes(infos[i].beta1), bytes(infos[i].tau2), bytes(infos[i].beta2), infos[i].name)
                   for i in range(min(held, cap))]
    rep.beacons = _beacons("groth16_ptau_beacons", ptau, cap)
    return rc == 1, rep


PTAU_VERIFY_KINDS = ("", "GENERATORS", "TAU_PAIR", "BETA_PAIR", "TAU_G1", "TAU_G2", "ALPHA_TAU", "BETA_TAU", "LAGRANGE_12", "LAGRANGE_13", "LAGRANGE_14",
                     "LAGRANGE_15", "POINT", "IDENTITY")


class PtauVerifyReport(C.Structure):
    """Groth16PtauVerifyReport: the power, whether sections 12 to 15 were there, the first failing kind, one bit per failing equation
    (bit kind − 1), the faulty point of POINT / IDENTITY (section, kind, lowest element), the points of sections 2 to 5 and 12 to 15,
    the stage times.  .kind_name and .failed: the kinds by name"""
    _fields_ = [("power", C.c_uint32), ("prepared", C.c_int32), ("kind", C.c_int32), ("failed_mask", C.c_uint32),
                ("fault_section", C.c_int32), ("fault_kind", C.c_int32), ("fault_index", C.c_uint64), ("points", C.c_uint64 * 8),
                ("upload_ms", C.c_double), ("device_ms", C.c_double), ("pairing_ms", C.c_double)]

    @property
    def kind_name(self):
        return PTAU_VERIFY_KINDS[self.kind] if 0 <= self.kind < len(PTAU_VERIFY_KINDS) else str(self.kind)

    @property
    def failed(self):
        return [PTAU_VERIFY_KINDS[k] for k in range(1, 12) if self.failed_mask >> (k - 1) & 1]


def ptau_verify(ptau, seed=None, device: str = "HIP"):
    """groth16_ptau_verify → (ok, PtauVerifyReport): are sections 2 to 6 of a powers-of-tau file the powers of one (tau, alpha, beta)
    and, when the file is prepared, sections 12 to 15 the transforms groth16_ptau_prepare writes?  ptau: the image, or a path that
    is mapped.  seed: 32 bytes for a reproducible run; None draws from the operating system, which is what soundness needs.  A
    faulty point or an identity in sections 2 to 6 is a verdict (ok False, kind POINT / IDENTITY), not an error.  It does NOT say who
    contributed: ptau_contributions does.  Raises ProverError (−2 a malformed container, −3 a power above 27)."""
    sd = _seed32(seed, "ptau_verify")
    rep = PtauVerifyReport()
    if _is_path(ptau):
        rc, what = lib().groth16_ptau_verify_file(os.fsencode(ptau), sd, device.encode(), C.byref(rep)), "ptau_verify_file"
    else:
        rc, what = lib().groth16_ptau_verify(_image(ptau), C.c_size_t(len(ptau)), sd, device.encode(), C.byref(rep)), "ptau_verify"
    if rc not in (0, 1):
        _pcheck(rc, what)
    return rc == 1, rep


def sum_commitments(blocks: bytes, count: int) -> bytes:
    out = (C.c_uint8 * COMMITMENTS_BYTES)()
    _pcheck(lib().groth16_sum_commitments(blocks, count, out), "sum_commitments")
    return bytes(out)


class PointsPackReport(C.Structure):
    """Groth16PointsPackReport: the element count, the lowest faulty element with its kind and how many are faulty, the stage times"""
    _fields_ = [("n", C.c_uint64), ("fault_kind", C.c_int32), ("fault_index", C.c_uint64), ("fault_count", C.c_uint64),
                ("upload_ms", C.c_double), ("device_ms", C.c_double), ("download_ms", C.c_double)]


class PtauPackReport(C.Structure):
    """Groth16PtauPackReport: power, prepared, the G1 and G2 point counts, the input's and the output's bytes, the first faulty
    section with its lowest faulty element, its kind and that section's fault count, the stage times"""
    _fields_ = [("power", C.c_uint32), ("prepared", C.c_int32), ("points", C.c_uint64 * 2), ("in_bytes", C.c_uint64), ("out_bytes", C.c_uint64),
                ("fault_section", C.c_int32), ("fault_kind", C.c_int32), ("fault_index", C.c_uint64), ("fault_count", C.c_uint64),
                ("upload_ms", C.c_double), ("device_ms", C.c_double), ("download_ms", C.c_double), ("write_ms", C.c_double)]


class PointFault(ProverError):
    """a faulty point refused by a pack / unpack call: .report says which"""
    report = None


def _fault_check(fault_type, rc, what, rep):
    """_pcheck, but a −2 whose report names a fault raises fault_type (a ProverError) carrying the report"""
    try:
        _pcheck(rc, what)
    except ProverError as e:
        if rc == -2 and rep.fault_kind:
            fault = fault_type(str(e))
            fault.report = rep
            raise fault from None
        raise


def _pack_check(rc, what, rep):
    _fault_check(PointFault, rc, what, rep)


def _points_call(entry, what, buf, in_elem, out_elem, g2, device):
    if len(buf) % in_elem:
        raise ValueError(f"{what}: {len(buf)} bytes are no multiple of {in_elem}")
    n = len(buf) // in_elem
    out, rep = C.create_string_buffer(max(n * out_elem, 1)), PointsPackReport()
    rc = entry(_image(buf) if n else None, C.c_uint64(n), C.c_int(1 if g2 else 0), out, device.encode(), C.byref(rep))
    _pack_check(rc, what, rep)
    return out.raw[:n * out_elem], rep


def points_pack(buf, g2: bool = False, device: str = "HIP"):
    """groth16_points_pack → (packed bytes, PointsPackReport): file-form points (64 bytes each, g2: 128; affine, Montgomery form, the
    identity all zero) as x and one bit of y, 32 or 64 bytes each, on the GPU.  Every point passes the key tools' lane test first;
    a faulty one raises PointFault (−2) whose .report names the lowest faulty element, its kind and the count.  An empty buffer is valid."""
    return _points_call(lib().groth16_points_pack, "points_pack", buf, 128 if g2 else 64, 64 if g2 else 32, g2, device)


def points_unpack(buf, g2: bool = False, device: str = "HIP"):
    """groth16_points_unpack → (file-form points, PointsPackReport): the inverse of points_pack, a square root per point on the GPU.
    A word that is no valid packed point raises PointFault (−2): flags, x >= q, no point with this x, outside the subgroup (G2)."""
    return _points_call(lib().groth16_points_unpack, "points_unpack", buf, 64 if g2 else 32, 128 if g2 else 64, g2, device)


def ptau_packed_size(power: int, prepared: bool, ptau_bytes: int) -> int:
    """groth16_ptau_packed_size: the bytes of ptau_pack's file for a .ptau of this power, form and size; host only.  Raises
    ProverError −3 for a power above 27 or a size below the form's point sections."""
    size = C.c_uint64()
    _pcheck(lib().groth16_ptau_packed_size(C.c_uint32(power), C.c_int(1 if prepared else 0), C.c_uint64(ptau_bytes), C.byref(size)), "ptau_packed_size")
    return size.value


def ptau_unpacked_size(power: int, prepared: bool, packed_bytes: int) -> int:
    """groth16_ptau_unpacked_size: the bytes of the .ptau that ptau_unpack writes for a packed file of this power, form and size"""
    size = C.c_uint64()
    _pcheck(lib().groth16_ptau_unpacked_size(C.c_uint32(power), C.c_int(1 if prepared else 0), C.c_uint64(packed_bytes), C.byref(size)), "ptau_unpacked_size")
    return size.value


def _ptau_transcode(what, buffer_entry, file_entry, src, out, device):
    rep = PtauPackReport()
    if _path_or_image(what, src, out):
        _pack_check(file_entry(os.fsencode(src), os.fsencode(out), device.encode(), C.byref(rep)), what + "_file", rep)
        return None, rep
    buf = _sized_twice(lambda buf, room: buffer_entry(_image(src), C.c_size_t(len(src)), buf, room, device.encode(), C.byref(rep)), rep, "out_bytes", what, _pack_check)
    return buf.raw[:rep.out_bytes], rep


def ptau_pack(ptau, out=None, device: str = "HIP"):
    """groth16_ptau_pack → (packed bytes | None, PtauPackReport): a .ptau, unprepared or prepared, with every point as x and one bit
    of y — half the bytes, magic "ptaz" (include/groth16_prover.h has the form).  ptau: the image, and the packed file comes back as
    bytes; or a path together with `out`, the path the packed file is written to (a temporary, renamed).  Every point passes the
    lane tests first: PointFault (−2) "ptau: section S, element E: kind", its .report saying the same, and nothing written."""
    return _ptau_transcode("ptau_pack", lib().groth16_ptau_pack, lib().groth16_ptau_pack_file, ptau, out, device)


def ptau_unpack(packed, out=None, device: str = "HIP"):
    """groth16_ptau_unpack → (ptau bytes | None, PtauPackReport): the .ptau a packed file came from, byte for byte: a square root per
    point on the GPU, which is also the on-curve test.  Arguments and errors as ptau_pack."""
    return _ptau_transcode("ptau_unpack", lib().groth16_ptau_unpack, lib().groth16_ptau_unpack_file, packed, out, device)


class PtauTruncateReport(C.Structure):
    """Groth16PtauTruncateReport: the input's and the output's power, prepared, the elements of section 12's block power_out + 1 that
    were fixed up, the input's and the output's bytes, the faulty section with its lowest faulty element, its kind and the count,
    the stage times"""
    _fields_ = [("power_in", C.c_uint32), ("power_out", C.c_uint32), ("prepared", C.c_int32), ("points_fixed", C.c_uint64), ("in_bytes", C.c_uint64),
                ("out_bytes", C.c_uint64), ("fault_section", C.c_int32), ("fault_kind", C.c_int32), ("fault_index", C.c_uint64), ("fault_count", C.c_uint64),
                ("upload_ms", C.c_double), ("device_ms", C.c_double), ("download_ms", C.c_double), ("write_ms", C.c_double)]


def ptau_truncated_size(ptau, power: int) -> int:
    """groth16_ptau_truncated_size: the bytes of ptau_truncate's file for this .ptau (unprepared or prepared) and power; host only.
    Raises ProverError −3 for a power above the file's, −2 for a malformed container."""
    size = C.c_uint64()
    _pcheck(lib().groth16_ptau_truncated_size(_image(ptau), C.c_size_t(len(ptau)), C.c_uint32(power), C.byref(size)), "ptau_truncated_size")
    return size.value


def ptau_truncate(ptau, power: int, out=None, device: str = "HIP"):
    """groth16_ptau_truncate → (ptau bytes | None, PtauTruncateReport): the file of power `power` <= the input's — prefixes of the
    sections, section 1 with the new power, and for a prepared input section 12's block power + 1 fixed up on the GPU so that the
    result is what ptau_prepare writes for the truncated unprepared file (include/groth16_prover.h).  ptau: the image, and the file
    comes back as bytes; or a path together with `out`, the path the file is written to (a temporary, renamed).  An unprepared
    input, or power equal to the file's, opens no GPU.  A faulty point of the block or of the one point of section 2 that is read
    raises PointFault (−2) with .report, and nothing is written; the copied prefixes are not tested (ptau_verify judges a file)."""
    rep = PtauTruncateReport()
    if _path_or_image("ptau_truncate", ptau, out):
        _pack_check(lib().groth16_ptau_truncate_file(os.fsencode(ptau), os.fsencode(out), C.c_uint32(power), device.encode(), C.byref(rep)), "ptau_truncate_file", rep)
        return None, rep
    size = ptau_truncated_size(ptau, power)
    buf = C.create_string_buffer(size)
    _pack_check(lib().groth16_ptau_truncate(_image(ptau), C.c_size_t(len(ptau)), C.c_uint32(power), buf, C.c_size_t(size), device.encode(), C.byref(rep)), "ptau_truncate", rep)
    return buf.raw[:rep.out_bytes], rep


class WtnsPackReport(C.Structure):
    """Groth16WtnsPackReport: the value count, the input's and the output's bytes, the lowest faulty element with its kind and how
    many are faulty, the stage times (device entries)"""
    _fields_ = [("n_witness", C.c_uint32), ("in_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("fault_kind", C.c_int32), ("fault_index", C.c_uint64),
                ("fault_count", C.c_uint64), ("upload_ms", C.c_double), ("kernel_ms", C.c_double), ("device_ms", C.c_double), ("download_ms", C.c_double),
                ("write_ms", C.c_double)]


WTNZ_KINDS = ("", "CODE", "NONCANONICAL", "RANGE", "DIRECTORY")


class WitnessFault(ProverError):
    """a value refused by wtns_pack / wtns_unpack: .report names the lowest faulty element, its kind and the count"""
    report = None


def _wtns_check(rc, what, rep):
    _fault_check(WitnessFault, rc, what, rep)


def _wtns_transcode(what, buffer_call, file_call, src, out):
    rep = WtnsPackReport()
    if _path_or_image(what, src, out):
        _wtns_check(file_call(os.fsencode(src), os.fsencode(out), C.byref(rep)), what + "_file", rep)
        return None, rep
    buf = _sized_twice(lambda buf, room: buffer_call(_image(src), C.c_size_t(len(src)), buf, room, C.byref(rep)), rep, "out_bytes", what, _wtns_check)
    return buf.raw[:rep.out_bytes], rep


def wtns_packed_size(wtns) -> int:
    """groth16_wtns_packed_size: the bytes of wtns_pack's output for this .wtns image; host only"""
    size = C.c_uint64()
    _pcheck(lib().groth16_wtns_packed_size(_image(wtns), C.c_size_t(len(wtns)), C.byref(size)), "wtns_packed_size")
    return size.value


def wtns_pack(wtns, out=None):
    """groth16_wtns_pack → (packed bytes | None, WtnsPackReport): a .wtns with a code byte per value and only the value's significant
    bytes, magic "wtnz" (include/groth16_prover.h has the form); host only: needs no GPU.  wtns: the image, and the packed witness
    comes back as bytes; or a path together with `out`, the path it is written to.  A value >= r raises WitnessFault (−2)."""
    return _wtns_transcode("wtns_pack", lib().groth16_wtns_pack, lib().groth16_wtns_pack_file, wtns, out)


def wtns_unpack(packed, out=None, device=None):
    """groth16_wtns_unpack_host (device=None: on the host, no GPU is initialised) or groth16_wtns_unpack (device="HIP": sections 2 to
    4 go up, one kernel decodes them) → (.wtns bytes | None, WtnsPackReport).  packed / out as wtns_pack.  A faulty value raises
    WitnessFault (−2 "wtnz: element E: kind"), its .report naming the lowest faulty element and the count; nothing is written."""
    if device is None:
        return _wtns_transcode("wtns_unpack_host", lib().groth16_wtns_unpack_host, lib().groth16_wtns_unpack_host_file, packed, out)
    dev = device.encode()
    return _wtns_transcode("wtns_unpack", lambda p, n, o, c, r: lib().groth16_wtns_unpack(p, n, o, c, dev, r),
                           lambda i, o, r: lib().groth16_wtns_unpack_file(i, o, dev, r), packed, out)


class ZkeyPackReport(C.Structure):
    """Groth16ZkeyPackReport: the header's counts, the G1 and G2 point counts, the input's and the output's bytes, the packed point
    sections' and the packed section 4's bytes, the first faulty section with its lowest faulty element, its kind and that section's
    fault count, the stage times"""
    _fields_ = [("n_vars", C.c_uint32), ("n_public", C.c_uint32), ("domain", C.c_uint32), ("n_coef", C.c_uint32), ("points", C.c_uint64 * 2),
                ("in_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("point_bytes", C.c_uint64), ("coef_bytes", C.c_uint64),
                ("fault_section", C.c_int32), ("fault_kind", C.c_int32), ("fault_index", C.c_uint64), ("fault_count", C.c_uint64),
                ("upload_ms", C.c_double), ("device_ms", C.c_double), ("download_ms", C.c_double), ("write_ms", C.c_double)]


class ZkeyCoefsReport(C.Structure):
    """Groth16ZkeyCoefsReport: the record count, the input's and the output's bytes, the lowest faulty coefficient with its kind
    (WTNZ_KINDS) and how many are faulty, the stage times"""
    _fields_ = [("n", C.c_uint64), ("in_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("fault_kind", C.c_int32), ("fault_index", C.c_uint64),
                ("fault_count", C.c_uint64), ("upload_ms", C.c_double), ("device_ms", C.c_double), ("download_ms", C.c_double)]


class KeyFault(ProverError):
    """a point or a coefficient refused by zkey_pack / zkey_unpack / coefs_pack / coefs_unpack: .report says which"""
    report = None


def _key_check(rc, what, rep):
    _fault_check(KeyFault, rc, what, rep)


def zkey_unpacked_size(zkez) -> int:
    """groth16_zkey_unpacked_size: the bytes of the .zkey a packed key came from, exact, from the container alone; host only"""
    size = C.c_uint64()
    _pcheck(lib().groth16_zkey_unpacked_size(_image(zkez), C.c_size_t(len(zkez)), C.byref(size)), "zkey_unpacked_size")
    return size.value


def zkey_packed_bound(zkey) -> int:
    """groth16_zkey_packed_bound: an upper bound of zkey_pack's output for this .zkey — every value at 32 bytes; host only"""
    size = C.c_uint64()
    _pcheck(lib().groth16_zkey_packed_bound(_image(zkey), C.c_size_t(len(zkey)), C.byref(size)), "zkey_packed_bound")
    return size.value


def _zkey_transcode(what, buffer_entry, file_entry, room, src, out, device):
    rep = ZkeyPackReport()
    if _path_or_image(what, src, out):
        _key_check(file_entry(os.fsencode(src), os.fsencode(out), device.encode(), C.byref(rep)), what + "_file", rep)
        return None, rep
    buf = C.create_string_buffer(max(room(src), 1))      # (a refused container raises here, with the reader's message)
    _key_check(buffer_entry(_image(src), C.c_size_t(len(src)), buf, C.c_size_t(len(buf)), device.encode(), C.byref(rep)), what, rep)
    return buf.raw[:rep.out_bytes], rep


def zkey_pack(zkey, out=None, device: str = "HIP"):
    """groth16_zkey_pack → (packed bytes | None, ZkeyPackReport): a .zkey with every point as x and one bit of y and every coefficient
    as a code byte and its significant bytes, magic "zkez" (include/groth16_prover.h has the form).  zkey: the image, and the packed
    key comes back as bytes; or a path together with `out`, the path the packed key is written to (a temporary, renamed).  Every point
    passes the lane tests first and every coefficient is below r: KeyFault (−2) "zkey: section S, element E: kind" / "zkey:
    coefficient E: not below r", its .report saying the same, and nothing written."""
    return _zkey_transcode("zkey_pack", lib().groth16_zkey_pack, lib().groth16_zkey_pack_file, zkey_packed_bound, zkey, out, device)


def zkey_unpack(zkez, out=None, device: str = "HIP"):
    """groth16_zkey_unpack → (.zkey bytes | None, ZkeyPackReport): the .zkey a packed key came from, byte for byte.  Arguments as
    zkey_pack; KeyFault (−2) "zkez: section S, element E: kind" / "zkez: coefficient E: kind"."""
    return _zkey_transcode("zkey_unpack", lib().groth16_zkey_unpack, lib().groth16_zkey_unpack_file, zkey_unpacked_size, zkez, out, device)


def coefs_pack(records, device: str = "HIP"):
    """groth16_zkey_coefs_pack → (the body of a packed section 4, ZkeyCoefsReport): n records of 44 bytes {m, c, s, value·R²} through
    the two pack kernels; declared_count = n.  A value not below r raises KeyFault (−2).  An empty buffer is valid."""
    if len(records) % 44:
        raise ValueError(f"coefs_pack: {len(records)} bytes are no multiple of 44")
    n = len(records) // 44
    buf, rep = C.create_string_buffer(24 + 45 * n + 8 * ((n + 255) // 256)), ZkeyCoefsReport()
    rc = lib().groth16_zkey_coefs_pack(_image(records) if n else None, C.c_uint64(n), buf, C.c_size_t(len(buf)), device.encode(), C.byref(rep))
    _key_check(rc, "coefs_pack", rep)
    return buf.raw[:rep.out_bytes], rep


def coefs_unpack(body, device: str = "HIP"):
    """groth16_zkey_coefs_unpack → (n records of 44 bytes, ZkeyCoefsReport): the inverse of coefs_pack.  The body passes the reader's
    tests of section 4 first (ProverError −2); a faulty value raises KeyFault (−2 "zkez: coefficient E: kind")."""
    rep = ZkeyCoefsReport()
    n = int.from_bytes(bytes(body[4:8]), "little") if len(body) >= 8 else 0
    buf = C.create_string_buffer(max(44 * n, 1))
    rc = lib().groth16_zkey_coefs_unpack(_image(body), C.c_size_t(len(body)), buf, C.c_size_t(44 * n), device.encode(), C.byref(rep))
    _key_check(rc, "coefs_unpack", rep)
    return buf.raw[:rep.out_bytes], rep
