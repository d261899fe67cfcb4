"""ctypes binding of the MI355X Noise ChaChaPoly engine (include/noise_gpu.h).

The product is the C ABI in noise-cpp_amd/lib/libnoise_amd.so (HIP kernels for
gfx950) and the C++20 noise::CipherState over it.  This module is the thin
Python view used by tests/, bench.py and __graft_entry__.py: it passes device
pointers (torch tensors on the GPU are used only as HBM allocations) and
streams straight through to the C ABI.  There is no Python or CPU compute
path: if the shared library is missing, load() raises.
"""
import ctypes
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", ".."))
PKG = os.path.join(ROOT, "noise-cpp_amd")
# NOISE_AMD_LIB: load another build of the library (A/B tuning runs only)
LIB_PATH = os.environ.get("NOISE_AMD_LIB") or os.path.join(PKG, "lib", "libnoise_amd.so")
HEADER = os.path.join(ROOT, "include", "noise_gpu.h")

OK, E_NONCE, E_MAC, E_ARG, E_HIP, E_NODEV = 0, 1, 2, 3, 4, 5
REC_OK, REC_BAD_MAC, REC_BAD_KEY, REC_NONCE = 0, 1, 2, 3
REC_REPLAY = 4
CS_WINDOW = 1024  # nonces per session's replay window (NOISE_GPU_CS_WINDOW)
REC_MALFORMED = 5  # datagram calls: bad packet length or type, payload over DGRAM_MAX_LEN
DGRAM_HDR, DGRAM_MAX_LEN = 16, 65519  # header bytes {LE32 type, LE32 receiver, LE64 counter}; payload limit
REC_EMPTY = 6  # stream-framing calls: a d_recs slot beyond the frames the call took
# per connection (noise_gpu_framed_*): open stopped at a length < 16; max_rec slots ran out; seal: a record refused
FRAMED_OK, FRAMED_BAD_LEN, FRAMED_FULL, FRAMED_REFUSED = 0, 1, 2, 3
FRAMED_MAX_PAYLOAD = 65519  # plaintext bytes of one frame: BE16(len + 16) <= 65535
NONCE_LIMIT = (1 << 64) - 2  # noise.cpp:398 refuses n == 2^64-2


class Record(ctypes.Structure):
    """noise_gpu_record (include/noise_gpu.h)."""
    _fields_ = [("in_off", ctypes.c_uint64), ("out_off", ctypes.c_uint64),
                ("nonce", ctypes.c_uint64), ("ad_off", ctypes.c_uint64),
                ("len", ctypes.c_uint32), ("ad_len", ctypes.c_uint32),
                ("key_idx", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


RECORD_DTYPE = None  # numpy structured dtype, built lazily


def record_dtype():
    global RECORD_DTYPE
    if RECORD_DTYPE is None:
        import numpy as np
        RECORD_DTYPE = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("nonce", "<u8"),
                                 ("ad_off", "<u8"), ("len", "<u4"), ("ad_len", "<u4"),
                                 ("key_idx", "<u4"), ("reserved", "<u4")])
        assert RECORD_DTYPE.itemsize == ctypes.sizeof(Record) == 48
    return RECORD_DTYPE


class Span(ctypes.Structure):
    """noise_gpu_span (include/noise_gpu.h): per-session byte ranges."""
    _fields_ = [("base", ctypes.c_void_p), ("off", ctypes.c_void_p), ("stride", ctypes.c_uint64),
                ("len", ctypes.c_void_p), ("len_all", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class HsInfo(ctypes.Structure):
    """noise_gpu_hs_info (include/noise_gpu.h)."""
    _fields_ = [("message_index", ctypes.c_uint32), ("message_count", ctypes.c_uint32),
                ("my_turn", ctypes.c_int32), ("finished", ctypes.c_int32),
                ("overhead", ctypes.c_uint32), ("psk_count", ctypes.c_uint32)]


HS_S, HS_E, HS_RS, HS_RE = 0, 1, 2, 3
HS_OK, HS_BAD_MAC, HS_BAD_LEN = 0, 1, 3


class NoiseGpuError(RuntimeError):
    def __init__(self, code, what):
        super().__init__("%s (status %d): %s" % (what, code, _lib.noise_gpu_last_error().decode()
                                                if _lib else ""))
        self.code = code


_lib = None
u8p, u64, u32, vp = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p


def declared_symbols():
    """Function names declared in include/noise_gpu.h."""
    text = open(HEADER).read()
    return sorted(set(re.findall(r"^(?:int|const char \*)\s*(noise_gpu_\w+)\s*\(", text, re.M)))


def load(path=LIB_PATH):
    """Load the engine library (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise FileNotFoundError("libnoise_amd.so not built (%s); run __graft_entry__.build()" % path)
    lib = ctypes.CDLL(path)
    sig = {
        "noise_gpu_version": (ctypes.c_char_p, []),
        "noise_gpu_strerror": (ctypes.c_char_p, [ctypes.c_int]),
        "noise_gpu_last_error": (ctypes.c_char_p, []),
        "noise_gpu_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
        "noise_gpu_encrypt_uniform": (ctypes.c_int, [ctypes.c_char_p, u64, u8p, u64, u8p, u64, u32,
                                                     u8p, u64, u32, u64, vp]),
        "noise_gpu_decrypt_uniform": (ctypes.c_int, [ctypes.c_char_p, u64, u8p, u64, u8p, u64, u32,
                                                     u8p, u64, u32, u8p, u64, vp]),
        "noise_gpu_encrypt_records": (ctypes.c_int, [u8p, u32, u8p, u64, u8p, u8p, u8p, vp]),
        "noise_gpu_decrypt_records": (ctypes.c_int, [u8p, u32, u8p, u64, u8p, u8p, u8p, u8p, vp]),
        "noise_gpu_rekey_keys": (ctypes.c_int, [u8p, u64, vp]),
        "noise_gpu_x25519": (ctypes.c_int, [u8p, u8p, u8p, u64, vp]),
        "noise_gpu_encrypt_sessions": (ctypes.c_int, [u8p, u32, u8p, u8p, u8p, u64, u8p, u64, u32,
                                                      u64, vp]),
        "noise_gpu_decrypt_sessions": (ctypes.c_int, [u8p, u32, u8p, u8p, u8p, u64, u8p, u64, u32,
                                                      u8p, u64, vp]),
        "noise_gpu_encrypt_host": (ctypes.c_int, [ctypes.c_char_p, u64, u8p, ctypes.c_size_t,
                                                  u8p, ctypes.c_size_t]),
        "noise_gpu_decrypt_host": (ctypes.c_int, [ctypes.c_char_p, u64, u8p, ctypes.c_size_t,
                                                  u8p, ctypes.c_size_t]),
        "noise_gpu_rekey_host": (ctypes.c_int, [u8p]),
        "noise_gpu_encrypt_records_host": (ctypes.c_int, [u8p, u32, u8p, u64, u8p, u64, u8p, u64,
                                                          u8p, u64]),
        "noise_gpu_decrypt_records_host": (ctypes.c_int, [u8p, u32, u8p, u64, u8p, u64, u8p, u64,
                                                          u8p, u64, u8p]),
        "noise_gpu_encrypt_uniform_host": (ctypes.c_int, [ctypes.c_char_p, u64, u8p, u64, u8p, u64,
                                                          u32, u64, ctypes.POINTER(ctypes.c_double)]),
        "noise_gpu_decrypt_uniform_host": (ctypes.c_int, [ctypes.c_char_p, u64, u8p, u64, u8p, u64,
                                                          u32, u8p, u64,
                                                          ctypes.POINTER(ctypes.c_double)]),
        "noise_gpu_ctx_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
        "noise_gpu_ctx_destroy": (ctypes.c_int, [vp]),
        "noise_gpu_ctx_device": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_int)]),
        "noise_gpu_ctx_encrypt_host": (ctypes.c_int, [vp, ctypes.c_char_p, u64, u8p, ctypes.c_size_t,
                                                      u8p, ctypes.c_size_t]),
        "noise_gpu_ctx_decrypt_host": (ctypes.c_int, [vp, ctypes.c_char_p, u64, u8p, ctypes.c_size_t,
                                                      u8p, ctypes.c_size_t]),
        "noise_gpu_ctx_rekey_host": (ctypes.c_int, [vp, u8p]),
        "noise_gpu_ctx_encrypt_records_host": (ctypes.c_int, [vp, u8p, u32, u8p, u64, u8p, u64, u8p,
                                                              u64, u8p, u64]),
        "noise_gpu_ctx_decrypt_records_host": (ctypes.c_int, [vp, u8p, u32, u8p, u64, u8p, u64, u8p,
                                                              u64, u8p, u64, u8p]),
        "noise_gpu_ctx_encrypt_uniform_host": (ctypes.c_int, [vp, ctypes.c_char_p, u64, u8p, u64, u8p,
                                                              u64, u32, u64,
                                                              ctypes.POINTER(ctypes.c_double)]),
        "noise_gpu_ctx_decrypt_uniform_host": (ctypes.c_int, [vp, ctypes.c_char_p, u64, u8p, u64, u8p,
                                                              u64, u32, u8p, u64,
                                                              ctypes.POINTER(ctypes.c_double)]),
        "noise_gpu_set_resident": (ctypes.c_int, [ctypes.c_int, u32]),
        "noise_gpu_ctx_set_resident": (ctypes.c_int, [vp, ctypes.c_int, u32]),
        "noise_gpu_thread_release": (ctypes.c_int, []),
        "noise_gpu_fill_synthetic": (ctypes.c_int, [u8p, u64, u64, u64, vp]),
        "noise_gpu_scratch_wipe": (ctypes.c_int, [vp]),
        "noise_gpu_scratch_release": (ctypes.c_int, [vp]),
        "noise_gpu_hs_create": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, u64,
                                               ctypes.POINTER(ctypes.c_void_p)]),
        "noise_gpu_hs_destroy": (ctypes.c_int, [vp]),
        "noise_gpu_hs_info_get": (ctypes.c_int, [vp, ctypes.POINTER(HsInfo)]),
        "noise_gpu_hs_set_key": (ctypes.c_int, [vp, ctypes.c_int, u8p, u64, vp]),
        "noise_gpu_hs_set_psks": (ctypes.c_int, [vp, u8p, vp]),
        "noise_gpu_hs_start": (ctypes.c_int, [vp, ctypes.POINTER(Span), vp]),
        "noise_gpu_hs_write_message": (ctypes.c_int, [vp, ctypes.POINTER(Span), ctypes.POINTER(Span),
                                                      u8p, vp]),
        "noise_gpu_hs_read_message": (ctypes.c_int, [vp, ctypes.POINTER(Span), ctypes.POINTER(Span),
                                                     u8p, u8p, vp]),
        "noise_gpu_hs_status": (ctypes.c_int, [vp, u8p, vp]),
        "noise_gpu_hs_split": (ctypes.c_int, [vp, u8p, u8p, u8p, u8p, vp]),
        "noise_gpu_cs_create": (ctypes.c_int, [u64, ctypes.POINTER(ctypes.c_void_p)]),
        "noise_gpu_cs_destroy": (ctypes.c_int, [vp]),
        "noise_gpu_cs_set": (ctypes.c_int, [vp, u64, u64, u8p, u64, u8p, vp]),
        "noise_gpu_cs_get": (ctypes.c_int, [vp, u64, u64, u8p, u8p, vp]),
        "noise_gpu_cs_rekey": (ctypes.c_int, [vp, u8p, u64, vp]),
        "noise_gpu_cs_assign": (ctypes.c_int, [vp, u8p, u64, u8p, u64, u8p, u64, vp]),
        "noise_gpu_cs_encrypt_records": (ctypes.c_int, [vp, u8p, u64, u8p, u8p, u8p, u8p, u64, vp]),
        "noise_gpu_cs_decrypt_records": (ctypes.c_int, [vp, u8p, u64, u8p, u8p, u8p, u8p, u64, vp]),
        "noise_gpu_cs_encrypt_sessions": (ctypes.c_int, [vp, u8p, u8p, u64, u8p, u64, u32, u8p, u64,
                                                         vp]),
        "noise_gpu_cs_decrypt_sessions": (ctypes.c_int, [vp, u8p, u8p, u64, u8p, u64, u32, u8p, u64,
                                                         vp]),
        "noise_gpu_csrekey_set": (ctypes.c_int, [vp, u64]),
        "noise_gpu_csrekey_get": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_uint64)]),
        "noise_gpu_cswin_reset": (ctypes.c_int, [vp, u64, u64, vp]),
        "noise_gpu_cswin_get": (ctypes.c_int, [vp, u64, u64, u8p, u8p, vp]),
        "noise_gpu_cswin_filter": (ctypes.c_int, [vp, u8p, u64, u8p, u64, u8p, u64, vp]),
        "noise_gpu_cswin_commit": (ctypes.c_int, [vp, u8p, u64, u8p, u64, u8p, u64, vp]),
        "noise_gpu_cswin_decrypt_records": (ctypes.c_int, [vp, u8p, u64, u8p, u8p, u8p, u8p, u64, vp]),
        "noise_gpu_cswin_decrypt_sessions": (ctypes.c_int, [vp, u8p, u8p, u8p, u64, u8p, u64, u32, u8p,
                                                            u64, vp]),
        "noise_gpu_dgram_seal": (ctypes.c_int, [vp, u32, u8p, u8p, ctypes.POINTER(Span),
                                                ctypes.POINTER(Span), u8p, u8p, u8p, u64, u64, vp]),
        "noise_gpu_dgram_open": (ctypes.c_int, [vp, u32, ctypes.POINTER(Span), ctypes.POINTER(Span), u8p,
                                                u8p, u8p, u64, u64, vp]),
        "noise_gpu_framed_open": (ctypes.c_int, [vp, u8p, ctypes.POINTER(Span), ctypes.POINTER(Span), u8p, u8p,
                                                 u64, u8p, u8p, u8p, u8p, u8p, u8p, u8p, u64, u64, vp]),
        "noise_gpu_framed_seal": (ctypes.c_int, [vp, u8p, ctypes.POINTER(Span), ctypes.POINTER(Span), u32, u8p,
                                                 u8p, u64, u8p, u8p, u8p, u8p, u8p, u8p, u64, u64, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def _check(rc, what):
    if rc != OK:
        raise NoiseGpuError(rc, what)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    return ctypes.c_void_p(stream.cuda_stream)


def _key(key):
    key = bytes(key)
    if len(key) != 32:
        raise ValueError("key must be 32 bytes")
    return key


# ---- device-resident batches (torch uint8 CUDA tensors as HBM buffers) ----
def encrypt_uniform(key, nonce0, d_in, in_stride, d_out, out_stride, length, nrec,
                    d_ad=None, ad_stride=0, ad_len=0, stream=None, in_offset=0, out_offset=0):
    lib = load()
    rc = lib.noise_gpu_encrypt_uniform(_key(key), nonce0 % (1 << 64),
                                       ctypes.c_void_p(d_in.data_ptr() + in_offset), in_stride,
                                       ctypes.c_void_p(d_out.data_ptr() + out_offset), out_stride,
                                       length, _ptr(d_ad), ad_stride, ad_len, nrec, _stream(stream))
    _check(rc, "noise_gpu_encrypt_uniform")


def decrypt_uniform(key, nonce0, d_in, in_stride, d_out, out_stride, length, d_status, nrec,
                    d_ad=None, ad_stride=0, ad_len=0, stream=None, in_offset=0, out_offset=0):
    lib = load()
    rc = lib.noise_gpu_decrypt_uniform(_key(key), nonce0 % (1 << 64),
                                       ctypes.c_void_p(d_in.data_ptr() + in_offset), in_stride,
                                       ctypes.c_void_p(d_out.data_ptr() + out_offset), out_stride,
                                       length, _ptr(d_ad), ad_stride, ad_len, _ptr(d_status), nrec,
                                       _stream(stream))
    _check(rc, "noise_gpu_decrypt_uniform")


def encrypt_records(d_keys, nkeys, d_recs, nrec, d_in, d_out, d_ad=None, stream=None):
    rc = load().noise_gpu_encrypt_records(_ptr(d_keys), nkeys, _ptr(d_recs), nrec, _ptr(d_in),
                                          _ptr(d_out), _ptr(d_ad), _stream(stream))
    _check(rc, "noise_gpu_encrypt_records")


def decrypt_records(d_keys, nkeys, d_recs, nrec, d_in, d_out, d_status, d_ad=None, stream=None):
    rc = load().noise_gpu_decrypt_records(_ptr(d_keys), nkeys, _ptr(d_recs), nrec, _ptr(d_in),
                                          _ptr(d_out), _ptr(d_ad), _ptr(d_status), _stream(stream))
    _check(rc, "noise_gpu_decrypt_records")


def encrypt_sessions(d_keys, nkeys, d_key_idx, d_nonces, d_in, in_stride, d_out, out_stride,
                     length, nrec, stream=None):
    rc = load().noise_gpu_encrypt_sessions(_ptr(d_keys), nkeys, _ptr(d_key_idx), _ptr(d_nonces),
                                           _ptr(d_in), in_stride, _ptr(d_out), out_stride, length,
                                           nrec, _stream(stream))
    _check(rc, "noise_gpu_encrypt_sessions")


def decrypt_sessions(d_keys, nkeys, d_key_idx, d_nonces, d_in, in_stride, d_out, out_stride,
                     length, d_status, nrec, stream=None):
    rc = load().noise_gpu_decrypt_sessions(_ptr(d_keys), nkeys, _ptr(d_key_idx), _ptr(d_nonces),
                                           _ptr(d_in), in_stride, _ptr(d_out), out_stride, length,
                                           _ptr(d_status), nrec, _stream(stream))
    _check(rc, "noise_gpu_decrypt_sessions")


def rekey_keys(d_keys, nkeys, stream=None):
    _check(load().noise_gpu_rekey_keys(_ptr(d_keys), nkeys, _stream(stream)), "noise_gpu_rekey_keys")


def x25519(d_scalars, d_points, d_out, n, stream=None):
    """d_out[i] = X25519(d_scalars[i], d_points[i] or 9): n x 32-byte device arrays."""
    _check(load().noise_gpu_x25519(_ptr(d_scalars), _ptr(d_points) if d_points is not None else None,
                                   _ptr(d_out), n, _stream(stream)), "noise_gpu_x25519")


def fill_synthetic(d_dst, nbytes, seed, offset=0, stream=None, dst_offset=0):
    rc = load().noise_gpu_fill_synthetic(ctypes.c_void_p(d_dst.data_ptr() + dst_offset), offset,
                                         nbytes, seed, _stream(stream))
    _check(rc, "noise_gpu_fill_synthetic")


def span(base, stride=0, length=0, off=None, lens=None):
    """A noise_gpu_span over torch device tensors (base: uint8, off: int64
    offsets, lens: int32 lengths; None = uniform stride / length)."""
    return Span(base.data_ptr(), None if off is None else off.data_ptr(), stride,
                None if lens is None else lens.data_ptr(), length, 0)


class HandshakeBatch:
    """n sessions of one handshake pattern in one role on the GPU
    (noise_gpu_hs_*): the batched form of noise::HandshakeState."""

    def __init__(self, pattern, initiator, n):
        self.lib, self.n = load(), n
        h = ctypes.c_void_p()
        _check(self.lib.noise_gpu_hs_create(pattern.encode(), 1 if initiator else 0, n,
                                            ctypes.byref(h)), "noise_gpu_hs_create")
        self.h = h

    def close(self):
        if self.h:
            _check(self.lib.noise_gpu_hs_destroy(self.h), "noise_gpu_hs_destroy")
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        i = HsInfo()
        _check(self.lib.noise_gpu_hs_info_get(self.h, ctypes.byref(i)), "noise_gpu_hs_info_get")
        return i

    def set_key(self, which, d_keys, stride=32, stream=None):
        _check(self.lib.noise_gpu_hs_set_key(self.h, which, _ptr(d_keys), stride, _stream(stream)),
               "noise_gpu_hs_set_key")

    def set_psks(self, d_psks, stream=None):
        _check(self.lib.noise_gpu_hs_set_psks(self.h, _ptr(d_psks), _stream(stream)),
               "noise_gpu_hs_set_psks")

    def start(self, prologue=None, stream=None):
        _check(self.lib.noise_gpu_hs_start(self.h, ctypes.byref(prologue) if prologue else None,
                                           _stream(stream)), "noise_gpu_hs_start")

    def write_message(self, msg, payload=None, d_msg_len=None, stream=None):
        _check(self.lib.noise_gpu_hs_write_message(
            self.h, ctypes.byref(payload) if payload else None, ctypes.byref(msg), _ptr(d_msg_len),
            _stream(stream)), "noise_gpu_hs_write_message")

    def read_message(self, msg, payload=None, d_payload_len=None, d_status=None, stream=None):
        _check(self.lib.noise_gpu_hs_read_message(
            self.h, ctypes.byref(msg), ctypes.byref(payload) if payload else None,
            _ptr(d_payload_len), _ptr(d_status), _stream(stream)), "noise_gpu_hs_read_message")

    def status(self, d_status, stream=None):
        _check(self.lib.noise_gpu_hs_status(self.h, _ptr(d_status), _stream(stream)),
               "noise_gpu_hs_status")

    def split(self, d_k1, d_k2, d_hash=None, d_rs=None, stream=None):
        _check(self.lib.noise_gpu_hs_split(self.h, _ptr(d_k1), _ptr(d_k2), _ptr(d_hash), _ptr(d_rs),
                                           _stream(stream)), "noise_gpu_hs_split")


class CipherStateTable:
    """nsess device-resident CipherStates (noise_gpu_cs_*): key rows and
    counters in HBM, nonces assigned on the GPU in the batch's record order.
    One stream at a time; tensors are HBM allocations (uint8 unless noted)."""

    RECORD_KEY_IDX_OFF, RECORD_NONCE_OFF = Record.key_idx.offset, Record.nonce.offset

    def __init__(self, nsess):
        self.lib, self.nsess = load(), nsess
        h = ctypes.c_void_p()
        _check(self.lib.noise_gpu_cs_create(nsess, ctypes.byref(h)), "noise_gpu_cs_create")
        self.h = h

    def close(self):
        if self.h:
            _check(self.lib.noise_gpu_cs_destroy(self.h), "noise_gpu_cs_destroy")
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set(self, first, count, d_keys, key_stride=32, d_n=None, stream=None):
        """d_keys: count key rows at key_stride (None: keep the keys); d_n:
        int64 tensor of count counters (None: 0)."""
        _check(self.lib.noise_gpu_cs_set(self.h, first, count, _ptr(d_keys), key_stride, _ptr(d_n),
                                         _stream(stream)), "noise_gpu_cs_set")

    def get(self, first, count, d_keys=None, d_n=None, stream=None):
        _check(self.lib.noise_gpu_cs_get(self.h, first, count, _ptr(d_keys), _ptr(d_n),
                                         _stream(stream)), "noise_gpu_cs_get")

    def rekey(self, d_sess=None, count=0, stream=None):
        """d_sess: int32 tensor of count session indices, or None: all."""
        _check(self.lib.noise_gpu_cs_rekey(self.h, _ptr(d_sess), count, _stream(stream)),
               "noise_gpu_cs_rekey")

    # ---- the in-band rekey schedule (noise_gpu_csrekey_*): REKEY whenever a
    # session's counter, after it moved, is a multiple of every
    def set_rekey_every(self, every):
        """0 = off.  The in-order and framed calls issued afterwards honour it;
        assign, the windowed and the datagram calls refuse a scheduled table."""
        _check(self.lib.noise_gpu_csrekey_set(self.h, every), "noise_gpu_csrekey_set")

    def rekey_every(self):
        every = ctypes.c_uint64(0)
        _check(self.lib.noise_gpu_csrekey_get(self.h, ctypes.byref(every)), "noise_gpu_csrekey_get")
        return every.value

    def assign(self, d_sess, d_nonce, nrec, d_status=None, sess_stride=4, nonce_stride=8,
               sess_offset=0, nonce_offset=0, stream=None):
        """Plain arrays (int32 sessions, int64 nonces) by default; for a
        descriptor array pass it as both d_sess and d_nonce with strides 48 and
        the offsets RECORD_KEY_IDX_OFF / RECORD_NONCE_OFF."""
        _check(self.lib.noise_gpu_cs_assign(
            self.h, ctypes.c_void_p(d_sess.data_ptr() + sess_offset), sess_stride,
            ctypes.c_void_p(d_nonce.data_ptr() + nonce_offset), nonce_stride, _ptr(d_status), nrec,
            _stream(stream)), "noise_gpu_cs_assign")

    def encrypt_records(self, d_recs, nrec, d_in, d_out, d_ad=None, d_status=None, len_sum=0,
                        stream=None):
        _check(self.lib.noise_gpu_cs_encrypt_records(
            self.h, _ptr(d_recs), nrec, _ptr(d_in), _ptr(d_out), _ptr(d_ad), _ptr(d_status), len_sum,
            _stream(stream)), "noise_gpu_cs_encrypt_records")

    def decrypt_records(self, d_recs, nrec, d_in, d_out, d_status, d_ad=None, len_sum=0, stream=None):
        _check(self.lib.noise_gpu_cs_decrypt_records(
            self.h, _ptr(d_recs), nrec, _ptr(d_in), _ptr(d_out), _ptr(d_ad), _ptr(d_status), len_sum,
            _stream(stream)), "noise_gpu_cs_decrypt_records")

    def encrypt_sessions(self, d_sess, d_in, in_stride, d_out, out_stride, length, nrec,
                         d_status=None, stream=None):
        _check(self.lib.noise_gpu_cs_encrypt_sessions(
            self.h, _ptr(d_sess), _ptr(d_in), in_stride, _ptr(d_out), out_stride, length,
            _ptr(d_status), nrec, _stream(stream)), "noise_gpu_cs_encrypt_sessions")

    def decrypt_sessions(self, d_sess, d_in, in_stride, d_out, out_stride, length, d_status, nrec,
                         stream=None):
        _check(self.lib.noise_gpu_cs_decrypt_sessions(
            self.h, _ptr(d_sess), _ptr(d_in), in_stride, _ptr(d_out), out_stride, length,
            _ptr(d_status), nrec, _stream(stream)), "noise_gpu_cs_decrypt_sessions")

    # ---- out-of-order receive: a replay window per session (noise_gpu_cswin_*)
    def window_reset(self, first, count, stream=None):
        _check(self.lib.noise_gpu_cswin_reset(self.h, first, count, _stream(stream)),
               "noise_gpu_cswin_reset")

    def window_get(self, first, count, d_next=None, d_bits=None, stream=None):
        """d_next: int64 tensor of count; d_bits: uint8 tensor of count 128-byte rows."""
        _check(self.lib.noise_gpu_cswin_get(self.h, first, count, _ptr(d_next), _ptr(d_bits),
                                            _stream(stream)), "noise_gpu_cswin_get")

    def _window_primitive(self, fn, name, d_sess, d_nonce, d_status, nrec, sess_stride, nonce_stride,
                          sess_offset, nonce_offset, stream):
        _check(fn(self.h, ctypes.c_void_p(d_sess.data_ptr() + sess_offset), sess_stride,
                  ctypes.c_void_p(d_nonce.data_ptr() + nonce_offset), nonce_stride, _ptr(d_status),
                  nrec, _stream(stream)), name)

    def window_filter(self, d_sess, d_nonce, d_status, nrec, sess_stride=4, nonce_stride=8,
                      sess_offset=0, nonce_offset=0, stream=None):
        """Addressing as assign(); read-only on the table."""
        self._window_primitive(self.lib.noise_gpu_cswin_filter, "noise_gpu_cswin_filter", d_sess,
                               d_nonce, d_status, nrec, sess_stride, nonce_stride, sess_offset,
                               nonce_offset, stream)

    def window_commit(self, d_sess, d_nonce, d_status, nrec, sess_stride=4, nonce_stride=8,
                      sess_offset=0, nonce_offset=0, stream=None):
        """d_status: REC_OK marks a verified record; the losers become REC_REPLAY."""
        self._window_primitive(self.lib.noise_gpu_cswin_commit, "noise_gpu_cswin_commit", d_sess,
                               d_nonce, d_status, nrec, sess_stride, nonce_stride, sess_offset,
                               nonce_offset, stream)

    def decrypt_records_window(self, d_recs, nrec, d_in, d_out, d_status, d_ad=None, len_sum=0,
                               stream=None):
        _check(self.lib.noise_gpu_cswin_decrypt_records(
            self.h, _ptr(d_recs), nrec, _ptr(d_in), _ptr(d_out), _ptr(d_ad), _ptr(d_status), len_sum,
            _stream(stream)), "noise_gpu_cswin_decrypt_records")

    def decrypt_sessions_window(self, d_sess, d_nonces, d_in, in_stride, d_out, out_stride, length,
                                d_status, nrec, stream=None):
        _check(self.lib.noise_gpu_cswin_decrypt_sessions(
            self.h, _ptr(d_sess), _ptr(d_nonces), _ptr(d_in), in_stride, _ptr(d_out), out_stride, length,
            _ptr(d_status), nrec, _stream(stream)), "noise_gpu_cswin_decrypt_sessions")

    # ---- the datagram wire format (noise_gpu_dgram_*): packets are a 16-byte
    # header {type, receiver, counter}, then ct || tag
    def seal_datagrams(self, type_, d_sess, payload, pkt, d_recs, d_status, nrec, d_peer=None,
                       d_pkt_len=None, len_sum=0, stream=None):
        """payload / pkt: span()s; d_sess: int32 sessions of this table; d_peer:
        int32 receiver index per session (None: the session index); d_recs: room
        for nrec descriptors (out); d_pkt_len: int32 (out, optional)."""
        _check(self.lib.noise_gpu_dgram_seal(
            self.h, type_, _ptr(d_sess), _ptr(d_peer), ctypes.byref(payload), ctypes.byref(pkt),
            _ptr(d_recs), _ptr(d_pkt_len), _ptr(d_status), len_sum, nrec, _stream(stream)),
            "noise_gpu_dgram_seal")

    def open_datagrams(self, type_, pkt, payload, d_recs, d_status, nrec, d_payload_len=None,
                       len_sum=0, stream=None):
        """pkt (with lengths) / payload: span()s; d_recs: room for nrec
        descriptors (out: receiver, counter, len, offsets); windowed receive."""
        _check(self.lib.noise_gpu_dgram_open(
            self.h, type_, ctypes.byref(pkt), ctypes.byref(payload), _ptr(d_recs), _ptr(d_payload_len),
            _ptr(d_status), len_sum, nrec, _stream(stream)), "noise_gpu_dgram_open")

    # ---- length-prefixed stream framing (noise_gpu_framed_*): connection j
    # carries frames BE16(len + 16) || ct || tag
    def open_framed(self, d_sess, wire, d_recs, d_status, max_rec, d_nframes, d_consumed, d_conn_status,
                    nconn, plain=None, d_first=None, d_first_bad=None, d_plain_len=None, d_total=None,
                    len_sum=0, stream=None):
        """wire (with lengths) / plain: span()s, plain None = in place; d_sess:
        int32 session per connection; d_recs / d_status: room for max_rec (out);
        d_nframes, d_first_bad: int32; d_first, d_consumed, d_plain_len, d_total:
        int64; d_conn_status: uint8 (FRAMED_*)."""
        _check(self.lib.noise_gpu_framed_open(
            self.h, _ptr(d_sess), ctypes.byref(wire), ctypes.byref(plain) if plain is not None else None,
            _ptr(d_recs), _ptr(d_status), max_rec, _ptr(d_first), _ptr(d_nframes), _ptr(d_first_bad),
            _ptr(d_consumed), _ptr(d_plain_len), _ptr(d_conn_status), _ptr(d_total), len_sum, nconn,
            _stream(stream)), "noise_gpu_framed_open")

    def seal_framed(self, d_sess, msg, wire, max_payload, d_recs, d_status, max_rec, d_nframes, d_msg_used,
                    d_wire_len, d_conn_status, nconn, d_first=None, d_total=None, len_sum=0, stream=None):
        """msg (with lengths) / wire: span()s; frame k of a connection lies at
        its wire offset + k * (max_payload + 18); arrays as open_framed."""
        _check(self.lib.noise_gpu_framed_seal(
            self.h, _ptr(d_sess), ctypes.byref(msg), ctypes.byref(wire), max_payload, _ptr(d_recs),
            _ptr(d_status), max_rec, _ptr(d_first), _ptr(d_nframes), _ptr(d_msg_used), _ptr(d_wire_len),
            _ptr(d_conn_status), _ptr(d_total), len_sum, nconn, _stream(stream)), "noise_gpu_framed_seal")


# ---- host-buffer entry points (CipherState single-record path) ------------
def encrypt_host(key, nonce, ad, plaintext):
    """ENCRYPT(k, n, ad, pt) through the GPU; returns ct || tag (bytes)."""
    buf = ctypes.create_string_buffer(bytes(plaintext), len(plaintext) + 16)
    adb = bytes(ad)
    rc = load().noise_gpu_encrypt_host(_key(key), nonce, adb or None, len(adb), buf, len(plaintext))
    _check(rc, "noise_gpu_encrypt_host")
    return buf.raw


def decrypt_host(key, nonce, ad, ciphertext):
    """DECRYPT through the GPU; returns plaintext or raises NoiseGpuError(E_MAC)."""
    ct = bytes(ciphertext)
    buf = ctypes.create_string_buffer(ct, max(len(ct), 1))
    adb = bytes(ad)
    rc = load().noise_gpu_decrypt_host(_key(key), nonce, adb or None, len(adb), buf, len(ct))
    _check(rc, "noise_gpu_decrypt_host")
    return buf.raw[:len(ct) - 16]


def rekey_host(key):
    buf = ctypes.create_string_buffer(_key(key), 32)
    _check(load().noise_gpu_rekey_host(buf), "noise_gpu_rekey_host")
    return buf.raw


def set_resident(on, idle_us=0):
    """Resident latency mode of the calling thread's single-record path
    (noise_gpu_set_resident): one workgroup stays on the GPU while on."""
    _check(load().noise_gpu_set_resident(1 if on else 0, idle_us), "noise_gpu_set_resident")


def thread_release():
    _check(load().noise_gpu_thread_release(), "noise_gpu_thread_release")


def version():
    return load().noise_gpu_version().decode()
