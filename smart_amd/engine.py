"""ctypes binding of libsmartgpu.so (include/smartgpu.h); Plan.launch, the call that sits in a caller's loop, goes
through the native extension smart_amd._fastcall (csrc/fastcall.cpp) where that was built.

Mirrors SMART's plugin surface: a *text* loaded once (smart.c:553-568,95-138),
*patterns* cut from it (smart.c:148-158), and per-algorithm `search` calls that
return an occurrence count plus preprocessing / searching times in ms
(main.h:28-39).  There is no CPU fallback here: if the HIP library cannot be
loaded or no device is present, calls raise SmartGpuError.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SMARTGPU_LIB overrides the library path (A/B runs of two builds in one session)
LIB_PATH = os.environ.get("SMARTGPU_LIB") or os.path.join(_HERE, "csrc", "libsmartgpu.so")
# the product library plus the superseded kernels (smartgpu_tune selects them): A/B tests and measurements
AB_LIB_PATH = os.path.join(_HERE, "csrc", "libsmartgpu_ab.so")
ALGOS = ("hor", "bm", "kmp", "so", "bndm", "epsm", "sa", "qs", "tunedbm", "raita", "hash3", "hash5", "hash8", "sbndm", "kr", "bndml")
# shortest pattern each algorithm applies to (the reference returns -1 below: raita.c:37, hash3.c:31, ...)
MIN_M = {"raita": 2, "hash3": 3, "hash5": 5, "hash8": 8, "sbndm": 2}

_lib = None


class SmartGpuError(RuntimeError):
    pass


# Plan.launch without ctypes: base types of Text and Plan that hold the handle (and the text's length) and call
# smartgpu_plan_launch through a pointer from the library that made the plan.  Where the extension is missing (no
# Python.h when the library was built, another interpreter) or SMARTGPU_BINDING=ctypes is set, launch is the
# pure-Python one below; nothing else depends on which of them runs.
_fastcall = None
if os.environ.get("SMARTGPU_BINDING", "native") != "ctypes":
    try:
        from . import _fastcall
    except ImportError:
        _fastcall = None
if _fastcall is not None:
    _fastcall.set_error_class(SmartGpuError)
_TextBase = _fastcall.TextBase if _fastcall else object
_PlanBase = _fastcall.PlanBase if _fastcall else object


def binding():
    """"native": Plan.launch is smart_amd._fastcall's; "ctypes": it is the pure-Python one."""
    return "native" if _fastcall else "ctypes"


def _addr(fn):
    return C.cast(fn, C.c_void_p).value


def _bind_text(text):
    """Hand a Text's base the entry point it needs, from the library that made the text; before `_h` is set."""
    if _fastcall:
        text._bind(_addr(text._L.smartgpu_text_length))


def _bind_plan(plan):
    if _fastcall:
        plan._bind(_addr(plan._L.smartgpu_plan_launch), _addr(plan._L.smartgpu_last_error))


def build():
    """Compile libsmartgpu.so for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-s", "-j", str(min(os.cpu_count() or 4, 12)), "-C", os.path.join(_HERE, "csrc")])


_loaded = {}


def use_library(path=None):
    """Make `path` (default: the product library) the library new Text / Plan objects and the module-level
    calls go to.  Objects made earlier keep the library that made them (they free through it)."""
    global _lib
    _lib = _load(path or LIB_PATH)
    return _lib


def lib():
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH)
    return _lib


def _load(path):
    if path in _loaded:
        return _loaded[path]
    if not os.path.exists(path):
        raise SmartGpuError("%s is missing: run `make -C smart_amd/csrc` (or __graft_entry__.build())" % path)
    # dmabuf IPC (the only mode this pool's driver supports) is an HSA flag read when the process first touches HIP:
    # set before the library — and through it ROCr — is loaded; the library's own constructor does the same for C callers
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    L = C.CDLL(path)
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    sig = {
        "smartgpu_version": (C.c_char_p, []),
        "smartgpu_last_error": (C.c_char_p, []),
        "smartgpu_device_count": (i32, []),
        "smartgpu_algo_id": (i32, [C.c_char_p]),
        "smartgpu_algo_name": (C.c_char_p, [i32]),
        "smartgpu_device_sync": (i32, [i32]),
        "smartgpu_text_upload": (vp, [vp, u64, i32]),
        "smartgpu_text_upload_tiled": (vp, [vp, u64, u64, u64, i32]),
        "smartgpu_text_generate": (vp, [u64, i32, u64, u64, i32]),
        "smartgpu_text_free": (None, [vp]),
        "smartgpu_text_length": (u64, [vp]),
        "smartgpu_text_device": (i32, [vp]),
        "smartgpu_text_read": (i32, [vp, u64, u64, vp]),
        "smartgpu_text_alphabet": (i32, [vp, vp]),
        "smartgpu_text_repeat_rate": (i32, [vp, C.POINTER(C.c_double)]),
        "smartgpu_search64": (i32, [i32, vp, u32, vp, u64, u64, C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "smartgpu_search_batch64": (i32, [i32, vp, u32, u32, vp, u64, u64, vp, vp, vp, C.POINTER(C.c_double)]),
        "smartgpu_search_batch64_each": (i32, [i32, vp, u32, u32, vp, u64, u64, vp, vp, vp, C.POINTER(C.c_double)]),
        "smartgpu_msearch_batch64": (i32, [i32, vp, u32, u32, vp, i32, vp, vp, C.POINTER(C.c_double)]),
        "smartgpu_find64": (i32, [vp, u32, vp, u64, u64, vp, u64, C.POINTER(u64)]),
        "smartgpu_find_batch64": (i32, [vp, u32, u32, vp, u64, u64, vp, u64, vp]),
        "smartgpu_last_times": (None, [C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "smartgpu_plan_create": (vp, [i32, vp, u32, i32]),
        "smartgpu_plan_free": (None, [vp]),
        "smartgpu_plan_launch": (i32, [vp, vp, u64, u64, i32, i32]),
        "smartgpu_plan_result": (i32, [vp, i32, C.POINTER(u64), C.POINTER(C.c_double)]),
        "smartgpu_plan_kernel_name": (C.c_char_p, [vp]),
        "smartgpu_kernel_for": (C.c_char_p, [i32, vp, u32]),
        "smartgpu_plan_result_device_ptr": (vp, [vp]),
        "smartgpu_build_table": (i32, [i32, vp, u32, vp, u32]),
        "smartgpu_plan_reset": (i32, [vp]),
        "smartgpu_plan_set_result_buffer": (i32, [vp, vp, i32]),
        "smartgpu_stream_mark": (i32, [i32, i32]),
        "smartgpu_stream_elapsed_ms": (i32, [i32, C.POINTER(C.c_double)]),
        "smartgpu_stream_handle": (vp, [i32]),
        "smartgpu_tune": (i32, [i32, i32]),
        "smartgpu_coalesce": (i32, [i32]),
        "smartgpu_coalesce_wide": (i32, [i32]),
        "smartgpu_coalesce_pass": (i32, [i32]),
        "smartgpu_coalesce_long": (C.c_longlong, [C.c_longlong]),
        "smartgpu_coalesce_stats": (i32, [i32, C.POINTER(u64), C.POINTER(u64)]),
        "smartgpu_coalesce_riders": (i32, [i32, C.POINTER(u64)]),
        "smartgpu_text_sampling": (C.c_longlong, [C.c_longlong]),
        "smartgpu_text_has_sample": (i32, [vp]),
        "smartgpu_coalesce_sample": (i32, [i32]),
        "smartgpu_coalesce_sampled": (i32, [i32, C.POINTER(u64)]),
        "smartgpu_coalesce_sample_grid": (i32, [i32]),
        "smartgpu_mtext_upload": (vp, [vp, u64, i32, vp]),
        "smartgpu_mtext_generate": (vp, [u64, i32, u64, i32, vp]),
        "smartgpu_mtext_free": (None, [vp]),
        "smartgpu_mtext_length": (u64, [vp]),
        "smartgpu_mtext_ngpus": (i32, [vp]),
        "smartgpu_mtext_partition": (i32, [u64, i32, i32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]),
        "smartgpu_selftest_launch_pool": (i32, [i32, i32]),
        "smartgpu_msearch64": (i32, [i32, vp, u32, vp, i32, C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "smartgpu_probe_read_ms": (i32, [vp, i32, C.POINTER(C.c_double)]),
        # packed texts (bit planes)
        "smartgpu_ptext_layout": (i32, [u64, i32, C.POINTER(i32), C.POINTER(u64)]),
        "smartgpu_ptext_pack": (vp, [vp]),
        "smartgpu_ptext_upload": (vp, [vp, u64, i32]),
        "smartgpu_ptext_free": (None, [vp]),
        "smartgpu_ptext_length": (u64, [vp]),
        "smartgpu_ptext_device": (i32, [vp]),
        "smartgpu_ptext_planes": (i32, [vp]),
        "smartgpu_ptext_bytes": (u64, [vp]),
        "smartgpu_ptext_symbols": (i32, [vp, vp]),
        "smartgpu_ptext_read": (i32, [vp, u64, u64, vp]),
        "smartgpu_ptext_probe_read_ms": (i32, [vp, i32, C.POINTER(C.c_double)]),
        "smartgpu_psearch64": (i32, [vp, u32, vp, u64, u64, C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "smartgpu_psearch_batch64": (i32, [vp, u32, u32, vp, u64, u64, vp, C.POINTER(C.c_double)]),
        "smartgpu_pfind64": (i32, [vp, u32, vp, u64, u64, vp, u64, C.POINTER(u64)]),
        "smartgpu_pfind_batch64": (i32, [vp, u32, u32, vp, u64, u64, vp, u64, vp]),
        "smartgpu_psearch_sets64": (i32, [vp, u32, vp, u64, u64, C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "smartgpu_pfind_sets64": (i32, [vp, u32, vp, u64, u64, vp, u64, C.POINTER(u64)]),
        "smartgpu_iupac_sets": (i32, [vp, i32, vp, u32, vp]),
        "smartgpu_psearch_mis64": (i32, [vp, u32, u32, vp, u64, u64, C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "smartgpu_pfind_mis64": (i32, [vp, u32, u32, vp, u64, u64, vp, vp, u64, C.POINTER(u64)]),
        "smartgpu_psearch_sets_mis64": (i32, [vp, u32, u32, vp, u64, u64, C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "smartgpu_pfind_sets_mis64": (i32, [vp, u32, u32, vp, u64, u64, vp, vp, u64, C.POINTER(u64)]),
        "smartgpu_psearch_edit64": (i32, [vp, u32, u32, vp, u64, u64, C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "smartgpu_pfind_edit64": (i32, [vp, u32, u32, vp, u64, u64, vp, vp, u64, C.POINTER(u64)]),
        "smartgpu_search_edit64": (i32, [vp, u32, u32, vp, u64, u64, C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "smartgpu_find_edit64": (i32, [vp, u32, u32, vp, u64, u64, vp, vp, u64, C.POINTER(u64)]),
        "smartgpu_search_edit_classes64": (i32, [vp, u32, u32, vp, u64, u64, C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "smartgpu_find_edit_classes64": (i32, [vp, u32, u32, vp, u64, u64, vp, vp, u64, C.POINTER(u64)]),
        "smartgpu_search_editl64": (i32, [vp, u32, u32, u32, vp, u64, u64, C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "smartgpu_find_editl64": (i32, [vp, u32, u32, u32, vp, u64, u64, vp, vp, u64, C.POINTER(u64)]),
        "smartgpu_search_editl_classes64": (i32, [vp, u32, u32, u32, vp, u64, u64, C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "smartgpu_find_editl_classes64": (i32, [vp, u32, u32, u32, vp, u64, u64, vp, vp, u64, C.POINTER(u64)]),
        "smartgpu_search_mis64": (i32, [vp, u32, u32, vp, u64, u64, C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "smartgpu_find_mis64": (i32, [vp, u32, u32, vp, u64, u64, vp, vp, u64, C.POINTER(u64)]),
        "smartgpu_search_mis_classes64": (i32, [vp, u32, u32, vp, u64, u64, C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "smartgpu_find_mis_classes64": (i32, [vp, u32, u32, vp, u64, u64, vp, vp, u64, C.POINTER(u64)]),
        "smartgpu_psearch_sets_edit64": (i32, [vp, u32, u32, vp, u64, u64, C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "smartgpu_pfind_sets_edit64": (i32, [vp, u32, u32, vp, u64, u64, vp, vp, u64, C.POINTER(u64)]),
        "smartgpu_psearch_editl64": (i32, [vp, u32, u32, u32, vp, u64, u64, C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "smartgpu_pfind_editl64": (i32, [vp, u32, u32, u32, vp, u64, u64, vp, vp, u64, C.POINTER(u64)]),
        "smartgpu_psearch_sets_editl64": (i32, [vp, u32, u32, u32, vp, u64, u64, C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "smartgpu_pfind_sets_editl64": (i32, [vp, u32, u32, u32, vp, u64, u64, vp, vp, u64, C.POINTER(u64)]),
        "smartgpu_palign_edit64": (i32, [vp, u32, u32, vp, u64, u64, vp, u64, vp, vp, vp]),
        "smartgpu_palign_sets_edit64": (i32, [vp, u32, u32, vp, u64, u64, vp, u64, vp, vp, vp]),
        "smartgpu_align_edit64": (i32, [vp, u32, u32, vp, u64, u64, vp, u64, vp, vp, vp]),
        "smartgpu_align_edit_classes64": (i32, [vp, u32, u32, vp, u64, u64, vp, u64, vp, vp, vp]),
        "smartgpu_align_editl64": (i32, [vp, u32, u32, vp, u64, u64, vp, u64, vp, vp, vp]),
        "smartgpu_align_editl_classes64": (i32, [vp, u32, u32, vp, u64, u64, vp, u64, vp, vp, vp]),
        "smartgpu_palign_editl64": (i32, [vp, u32, u32, vp, u64, u64, vp, u64, vp, vp, vp]),
        "smartgpu_palign_sets_editl64": (i32, [vp, u32, u32, vp, u64, u64, vp, u64, vp, vp, vp]),
        "smartgpu_iupac_revcomp": (i32, [vp, u32, vp]),
        # packed texts of five to eight values (three bit planes)
        "smartgpu_ptext_layout8": (i32, [u64, i32, C.POINTER(i32), C.POINTER(u64)]),
        "smartgpu_ptext_pack8": (vp, [vp]),
        "smartgpu_ptext_upload8": (vp, [vp, u64, i32]),
        "smartgpu_ptext_symbols8": (i32, [vp, vp]),
        "smartgpu_iupac_sets8": (i32, [vp, i32, vp, u32, vp]),
    }
    for a in ALGOS:
        sig["smartgpu_%s_search" % a] = (i32, [vp, i32, vp, i32])
    for name, (res, args) in sig.items():
        if not hasattr(L, name) and os.path.abspath(path) != os.path.join(_HERE, "csrc", "libsmartgpu.so"):
            continue  # an older build loaded for an A/B run (SMARTGPU_LIB / use_library): it lacks the newer entry points
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _loaded[path] = L
    return L


EXPORTS = None  # filled by tests from include/smartgpu.h


def _err(what):
    return SmartGpuError("%s: %s" % (what, lib().smartgpu_last_error().decode()))


def version():
    return lib().smartgpu_version().decode()


def device_count():
    return lib().smartgpu_device_count()


def algo_id(name):
    i = lib().smartgpu_algo_id(name.encode())
    if i < 0:
        raise SmartGpuError("unknown algorithm %r" % name)
    return i


def _u8(a):
    if isinstance(a, (bytes, bytearray)):
        a = np.frombuffer(bytes(a), dtype=np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8)


class Text(_TextBase):
    """A text resident in one GPU's HBM (the shmget/getText replacement)."""

    def __init__(self, handle):
        if not handle:
            raise _err("text")
        self._L = lib()  # the library that made the handle frees it
        _bind_text(self)
        self._h = handle

    @classmethod
    def upload(cls, data, device=0):
        data = _u8(data)
        return cls(lib().smartgpu_text_upload(data.ctypes.data, len(data), device))

    @classmethod
    def upload_tiled(cls, unit, n, phase=0, device=0):
        unit = _u8(unit)
        return cls(lib().smartgpu_text_upload_tiled(unit.ctypes.data, len(unit), phase, n, device))

    @classmethod
    def generate(cls, seed, sigma, n, off=0, device=0):
        return cls(lib().smartgpu_text_generate(seed, sigma, off, n, device))

    def __len__(self):
        return int(lib().smartgpu_text_length(self._h))

    @property
    def device(self):
        return lib().smartgpu_text_device(self._h)

    def read(self, off, length):
        out = np.empty(length, dtype=np.uint8)
        if lib().smartgpu_text_read(self._h, off, length, out.ctypes.data) != 0:
            raise _err("text_read")
        return out

    def alphabet(self):
        """The byte values the text holds, ascending (taken on the device when the text was created)."""
        bits = np.zeros(8, dtype=np.uint32)
        if lib().smartgpu_text_alphabet(self._h, bits.ctypes.data) != 0:
            raise _err("text_alphabet")
        return [c for c in range(256) if (int(bits[c >> 5]) >> (c & 31)) & 1]

    def repeat_rate(self):
        """How often two symbols of the text are equal (from a byte histogram of a sample, taken on the device when the
        text was created), or None where the text has no rate."""
        rate = C.c_double(-1.0)
        if lib().smartgpu_text_repeat_rate(self._h, C.byref(rate)) != 0:
            raise _err("text_repeat_rate")
        return rate.value if rate.value >= 0 else None

    def pattern(self, k, m):
        """P = T[k..k+m), as setOfRandomPatterns cuts it (smart.c:148-158)."""
        return self.read(k, m)

    def free(self):
        if self._h:
            self._L.smartgpu_text_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def ptext_layout(n, nvalues):
    """(planes, plane_bytes) of a packed text of n symbols over nvalues distinct byte values — smartgpu_ptext_layout,
    pure arithmetic, no device needed."""
    planes, nbytes = C.c_int(0), C.c_uint64(0)
    if lib().smartgpu_ptext_layout(n, nvalues, C.byref(planes), C.byref(nbytes)) != 0:
        raise _err("ptext_layout")
    return int(planes.value), int(nbytes.value)


def ptext_layout8(n, nvalues):
    """ptext_layout for 1 to 8 values — smartgpu_ptext_layout8: 1 / 2 / 3 planes for at most 2 / 4 / 8 values."""
    planes, nbytes = C.c_int(0), C.c_uint64(0)
    if lib().smartgpu_ptext_layout8(n, nvalues, C.byref(planes), C.byref(nbytes)) != 0:
        raise _err("ptext_layout8")
    return int(planes.value), int(nbytes.value)


class PackedText:
    """A text of at most four distinct byte values resident in one GPU's HBM as bit planes (smartgpu_ptext_*); with
    wide=True at most eight, five to eight of them on three planes (smartgpu_ptext_pack8 / smartgpu_ptext_upload8)."""

    def __init__(self, handle):
        if not handle:
            raise _err("packed text")
        self._h = handle
        self._L = lib()  # the library that made the handle frees it

    @classmethod
    def pack(cls, text, wide=False):
        """Packs a resident Text on the device; the Text stays valid and independent."""
        return cls((lib().smartgpu_ptext_pack8 if wide else lib().smartgpu_ptext_pack)(text._h))

    @classmethod
    def upload(cls, data, device=0, wide=False):
        data = _u8(data)
        return cls((lib().smartgpu_ptext_upload8 if wide else lib().smartgpu_ptext_upload)(data.ctypes.data, len(data), device))

    def __len__(self):
        return int(lib().smartgpu_ptext_length(self._h))

    @property
    def device(self):
        return lib().smartgpu_ptext_device(self._h)

    @property
    def planes(self):
        return lib().smartgpu_ptext_planes(self._h)

    @property
    def nbytes(self):
        """HBM bytes of the planes, pads excluded."""
        return int(lib().smartgpu_ptext_bytes(self._h))

    def symbols(self):
        """The byte values the text holds, ascending: symbols()[code] is the value of a code."""
        vals = np.zeros(8, dtype=np.uint8)
        k = lib().smartgpu_ptext_symbols8(self._h, vals.ctypes.data)
        if k < 0:
            raise _err("ptext_symbols")
        return [int(v) for v in vals[:k]]

    def read(self, off, length):
        out = np.empty(length, dtype=np.uint8)
        if lib().smartgpu_ptext_read(self._h, off, length, out.ctypes.data) != 0:
            raise _err("ptext_read")
        return out

    def iupac(self, pattern):
        """The sets of an IUPAC nucleotide pattern over this text's values: iupac_sets(pattern, self.symbols())."""
        return iupac_sets(pattern, self.symbols(), wide=True)

    def probe_read_gbs(self, reps=20):
        """Practical streaming-read rate (GB/s) of the device over the planes: the packed layout's roofline."""
        ms = C.c_double(0.0)
        if lib().smartgpu_ptext_probe_read_ms(self._h, reps, C.byref(ms)) != 0:
            raise _err("ptext_probe_read")
        return self.nbytes / (ms.value * 1e-3) / 1e9

    def free(self):
        if self._h:
            self._L.smartgpu_ptext_free(self._h)
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


class Plan(_PlanBase):
    """One (algorithm, pattern) preprocessed and resident on a device."""

    def __init__(self, algo, P, device=0):
        self.P = _u8(P)
        self.algo = algo
        self._L = lib()
        _bind_plan(self)
        self._h = self._L.smartgpu_plan_create(algo_id(algo), self.P.ctypes.data, len(self.P), device)
        if not self._h:
            raise _err("plan_create")

    def _launch_ctypes(self, text, slot=0, timed=False, off=0, n=None):
        if n is None:
            n = len(text) - off
        if lib().smartgpu_plan_launch(self._h, text._h, off, n, slot, 1 if timed else 0) != 0:
            raise _err("plan_launch")

    if _fastcall is None:
        launch = _launch_ctypes  # (otherwise _fastcall.PlanBase.launch, same signature)

    def result(self, slot=0):
        c = C.c_uint64(0)
        ms = C.c_double(0.0)
        if lib().smartgpu_plan_result(self._h, slot, C.byref(c), C.byref(ms)) != 0:
            raise _err("plan_result")
        return int(c.value), float(ms.value)

    def reset(self):
        if lib().smartgpu_plan_reset(self._h) != 0:
            raise _err("plan_reset")

    def set_result_buffer(self, device_ptr, nslots=1):
        if lib().smartgpu_plan_set_result_buffer(self._h, device_ptr, nslots) != 0:
            raise _err("plan_set_result_buffer")

    @property
    def kernel_name(self):
        return lib().smartgpu_plan_kernel_name(self._h).decode()

    @property
    def result_device_ptr(self):
        return lib().smartgpu_plan_result_device_ptr(self._h)

    def free(self):
        if self._h:
            self._L.smartgpu_plan_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MultiText:
    """A text sharded over several GPUs of this process (smartgpu_mtext_*)."""

    def __init__(self, handle):
        if not handle:
            raise _err("mtext")
        self._h = handle
        self._L = lib()

    @staticmethod
    def _devs(devices):
        if devices is None:
            return None, None
        arr = (C.c_int * len(devices))(*devices)
        return arr, C.cast(arr, C.c_void_p)

    @classmethod
    def upload(cls, data, ngpus, devices=None):
        data = _u8(data)
        keep, ptr = cls._devs(devices)
        return cls(lib().smartgpu_mtext_upload(data.ctypes.data, len(data), ngpus, ptr))

    @classmethod
    def generate(cls, seed, sigma, n, ngpus, devices=None):
        keep, ptr = cls._devs(devices)
        return cls(lib().smartgpu_mtext_generate(seed, sigma, n, ngpus, ptr))

    def __len__(self):
        return int(lib().smartgpu_mtext_length(self._h))

    def search(self, algo, P, reduce="rccl"):
        P = _u8(P)
        c = C.c_uint64(0)
        pre = C.c_double(0.0)
        run = C.c_double(0.0)
        rc = lib().smartgpu_msearch64(algo_id(algo), P.ctypes.data, len(P), self._h, 0 if reduce == "rccl" else 1,
                                      C.byref(c), C.byref(pre), C.byref(run))
        if rc != 0:
            raise _err("msearch64(%s) rc=%d" % (algo, rc))
        return int(c.value), float(pre.value), float(run.value)

    def search_batch(self, algo, patterns, reduce="rccl"):
        """(counts, pre_ms, batch_ms): every shard searched for all K patterns, ONE reduction of the K counts."""
        pats, ptrs, m = _pattern_set(patterns)
        K = len(pats)
        counts = np.zeros(K, dtype=np.uint64)
        pre = np.zeros(K, dtype=np.float64)
        batch = C.c_double(0.0)
        rc = lib().smartgpu_msearch_batch64(algo_id(algo), C.cast(ptrs, C.c_void_p), m, K, self._h, 0 if reduce == "rccl" else 1,
                                            counts.ctypes.data, pre.ctypes.data, C.byref(batch))
        if rc != 0:
            raise _err("msearch_batch64(%s) rc=%d" % (algo, rc))
        return counts, pre, float(batch.value)

    def free(self):
        if self._h:
            self._L.smartgpu_mtext_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def mtext_partition(n, ngpus, g):
    """(begin, own, held) of shard g of a text of n bytes over ngpus devices — smartgpu_mtext_partition, the arithmetic
    smartgpu_mtext_upload / _generate shard with; no device needed."""
    b, o, h = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    if lib().smartgpu_mtext_partition(n, ngpus, g, C.byref(b), C.byref(o), C.byref(h)) != 0:
        raise _err("mtext_partition")
    return int(b.value), int(o.value), int(h.value)


def search(algo, P, text, off=0, n=None):
    """(count, pre_ms, run_ms) of `algo` for P in text[off..off+n)."""
    P = _u8(P)
    if n is None:
        n = len(text) - off
    c = C.c_uint64(0)
    pre = C.c_double(0.0)
    run = C.c_double(0.0)
    rc = lib().smartgpu_search64(algo_id(algo), P.ctypes.data, len(P), text._h, off, n,
                                 C.byref(c), C.byref(pre), C.byref(run))
    if rc != 0:
        raise _err("search64(%s) rc=%d" % (algo, rc))
    return int(c.value), float(pre.value), float(run.value)


def _pcount(name, pat, ptext, off, n, *k):
    """(count, pre_ms, run_ms) of the packed count call smartgpu_<name>: `pat` the pattern or its sets, k the mismatches
    where the call takes them."""
    pat = _u8(pat)
    if n is None:
        n = len(ptext) - off
    c = C.c_uint64(0)
    pre = C.c_double(0.0)
    run = C.c_double(0.0)
    rc = getattr(lib(), "smartgpu_" + name)(pat.ctypes.data, len(pat), *k, ptext._h, off, n, C.byref(c), C.byref(pre), C.byref(run))
    if rc != 0:
        raise _err("%s rc=%d" % (name, rc))
    return int(c.value), float(pre.value), float(run.value)


def _pfind(name, pat, ptext, off, n, cap, *k):
    """(positions[, mismatches], count) of the packed find call smartgpu_<name>; the distances where the call takes k.
    More than `cap` occurrences (SMARTGPU_ERR_NOMEM with the count filled): None in place of the arrays."""
    pat = _u8(pat)
    if n is None:
        n = len(ptext) - off
    outs = [np.empty(max(cap, 1), dtype=dt) for dt in ((np.uint64, np.uint8) if k else (np.uint64,))]
    c = C.c_uint64(0)
    rc = getattr(lib(), "smartgpu_" + name)(pat.ctypes.data, len(pat), *k, ptext._h, off, n,
                                            *[o.ctypes.data if cap else None for o in outs], cap, C.byref(c))
    if rc == -5 and c.value > cap:
        return (None,) * len(outs) + (int(c.value),)
    if rc != 0:
        raise _err("%s rc=%d" % (name, rc))
    return tuple(o[:c.value].copy() for o in outs) + (int(c.value),)


def psearch(P, ptext, off=0, n=None):
    """(count, pre_ms, run_ms) of P in symbols [off, off+n) of a PackedText: the count by definition (bf.c:25-39)."""
    return _pcount("psearch64", P, ptext, off, n)


def psearch_batch(patterns, ptext, off=0, n=None):
    """(counts, batch_ms) of a pattern set of one length over a PackedText: K launches, one read-back."""
    pats, ptrs, m = _pattern_set(patterns)
    K = len(pats)
    if n is None:
        n = len(ptext) - off
    counts = np.zeros(K, dtype=np.uint64)
    batch = C.c_double(0.0)
    rc = lib().smartgpu_psearch_batch64(C.cast(ptrs, C.c_void_p), m, K, ptext._h, off, n, counts.ctypes.data, C.byref(batch))
    if rc != 0:
        raise _err("psearch_batch64 rc=%d" % rc)
    return counts, float(batch.value)


def pfind(P, ptext, off=0, n=None, cap=1 << 20):
    """(positions, count): the ascending start positions (relative to symbol 0) of P in symbols [off, off+n) of a
    PackedText, and their number — find() on a packed text.  When there are more than `cap`, positions is None and only
    the count is returned (smartgpu_pfind64 reports SMARTGPU_ERR_NOMEM; retry with cap >= count)."""
    return _pfind("pfind64", P, ptext, off, n, cap)


def pfind_batch(patterns, ptext, off=0, n=None, cap=1 << 20):
    """(list of K ascending uint64 arrays, counts) for a pattern set of one length over a PackedText; `cap` is the room for
    the positions of ALL patterns.  When they are more, the list is None and the counts say how much room a retry needs."""
    pats, ptrs, m = _pattern_set(patterns)
    K = len(pats)
    if n is None:
        n = len(ptext) - off
    out = np.empty(max(cap, 1), dtype=np.uint64)
    starts = np.zeros(K + 1, dtype=np.uint64)
    rc = lib().smartgpu_pfind_batch64(C.cast(ptrs, C.c_void_p), m, K, ptext._h, off, n, out.ctypes.data if cap else None, cap,
                                      starts.ctypes.data)
    counts = np.diff(starts)
    if rc == -5 and int(starts[K]) > cap:
        return None, counts
    if rc != 0:
        raise _err("pfind_batch64 rc=%d" % rc)
    return [out[int(starts[k]):int(starts[k + 1])].copy() for k in range(K)], counts


def psearch_sets(sets, ptext, off=0, n=None):
    """(count, pre_ms, run_ms) of a SET pattern in symbols [off, off+n) of a PackedText: sets[j] is a byte whose bit c says
    that position j accepts the symbol ptext.symbols()[c] (smartgpu_psearch_sets64; PackedText.iupac builds such sets)."""
    return _pcount("psearch_sets64", sets, ptext, off, n)


def pfind_sets(sets, ptext, off=0, n=None, cap=1 << 20):
    """(positions, count) of a SET pattern (psearch_sets) in symbols [off, off+n) of a PackedText, as pfind returns them:
    ascending, relative to symbol 0; positions is None when there are more than `cap`."""
    return _pfind("pfind_sets64", sets, ptext, off, n, cap)


def psearch_mis(P, ptext, k, off=0, n=None):
    """(count, pre_ms, run_ms) of the start positions in symbols [off, off+n) of a PackedText where P occurs with at most k
    mismatches (Hamming distance over bytes; 0 <= k <= 7; smartgpu_psearch_mis64).  A byte of P the text does not
    hold is a mismatch in every window."""
    return _pcount("psearch_mis64", P, ptext, off, n, k)


def pfind_mis(P, ptext, k, off=0, n=None, cap=1 << 20):
    """(positions, mismatches, count) of P with at most k mismatches (psearch_mis) in symbols [off, off+n) of a PackedText:
    the ascending start positions (uint64, relative to symbol 0), the distance of each (uint8) and their number;
    (None, None, count) when there are more than `cap`."""
    return _pfind("pfind_mis64", P, ptext, off, n, cap, k)


def psearch_sets_mis(sets, ptext, k, off=0, n=None):
    """(count, pre_ms, run_ms) of the start positions in symbols [off, off+n) of a PackedText where a SET pattern
    (psearch_sets) occurs with at most k mismatches — positions whose symbol is no member of the position's set; 0 <= k <= 7
    (smartgpu_psearch_sets_mis64).  A position with the empty set is a mismatch in every window."""
    return _pcount("psearch_sets_mis64", sets, ptext, off, n, k)


def pfind_sets_mis(sets, ptext, k, off=0, n=None, cap=1 << 20):
    """(positions, mismatches, count) of a SET pattern with at most k mismatches (psearch_sets_mis) in symbols [off, off+n)
    of a PackedText, as pfind_mis returns them; (None, None, count) when there are more than `cap`."""
    return _pfind("pfind_sets_mis64", sets, ptext, off, n, cap, k)


def psearch_edit(P, ptext, k, off=0, n=None):
    """(count, pre_ms, run_ms) of the END positions e in symbols [off, off+n) of a PackedText where P occurs within edit
    distance k — substitutions, insertions and deletions, 0 <= k <= 7, 1 <= len(P) <= 64 (smartgpu_psearch_edit64): some
    substring [s, e] of the range, off <= s, is at most k edits from P."""
    return _pcount("psearch_edit64", P, ptext, off, n, k)


def pfind_edit(P, ptext, k, off=0, n=None, cap=1 << 20):
    """(ends, distances, count) of P within edit distance k (psearch_edit) in symbols [off, off+n) of a PackedText: the
    ascending end positions (uint64, the match's last symbol, relative to symbol 0), the edit distance of each (uint8) and
    their number; (None, None, count) when there are more than `cap`."""
    return _pfind("pfind_edit64", P, ptext, off, n, cap, k)


def psearch_sets_edit(sets, ptext, k, off=0, n=None):
    """psearch_edit for a SET pattern (psearch_sets): a text symbol matches position j when its code is a member of sets[j]
    (smartgpu_psearch_sets_edit64).  An empty set matches nothing."""
    return _pcount("psearch_sets_edit64", sets, ptext, off, n, k)


def pfind_sets_edit(sets, ptext, k, off=0, n=None, cap=1 << 20):
    """(ends, distances, count) of a SET pattern within edit distance k (psearch_sets_edit), as pfind_edit returns them."""
    return _pfind("pfind_sets_edit64", sets, ptext, off, n, cap, k)


def psearch_editl(P, ptext, k, off=0, n=None, all_blocks=False):
    """psearch_edit for LONG patterns: 1 <= len(P) <= 256, 0 <= k <= 31 (smartgpu_psearch_editl64; Myers' recurrence in blocks
    of 32 rows with Ukkonen's cut-off).  all_blocks=True computes every block of every column (SMARTGPU_PEDITL_ALL_BLOCKS): the
    same answer, for cross-checks and measurements."""
    return _pcount("psearch_editl64", P, ptext, off, n, k, int(bool(all_blocks)))


def pfind_editl(P, ptext, k, off=0, n=None, cap=1 << 20, all_blocks=False):
    """(ends, distances, count) as pfind_edit returns them, for LONG patterns (psearch_editl; smartgpu_pfind_editl64)."""
    return _pfind("pfind_editl64", P, ptext, off, n, cap, k, int(bool(all_blocks)))


def psearch_sets_editl(sets, ptext, k, off=0, n=None, all_blocks=False):
    """psearch_editl for a SET pattern (psearch_sets_edit; smartgpu_psearch_sets_editl64)."""
    return _pcount("psearch_sets_editl64", sets, ptext, off, n, k, int(bool(all_blocks)))


def pfind_sets_editl(sets, ptext, k, off=0, n=None, cap=1 << 20, all_blocks=False):
    """(ends, distances, count) of a SET pattern within edit distance k, for LONG patterns (smartgpu_pfind_sets_editl64)."""
    return _pfind("pfind_sets_editl64", sets, ptext, off, n, cap, k, int(bool(all_blocks)))


def _palign(name, pat, ptext, k, ends, off, n, ops, words_per=3):
    pat = _u8(pat)
    if n is None:
        n = len(ptext) - off
    ends = np.ascontiguousarray(ends, dtype=np.uint64)
    count = len(ends)
    starts = np.empty(count, dtype=np.uint64)
    dist = np.empty(count, dtype=np.uint8)
    words = np.empty((count, words_per), dtype=np.uint64) if ops else None
    rc = getattr(lib(), "smartgpu_" + name)(pat.ctypes.data, len(pat), k, ptext._h, off, n, ends.ctypes.data if count else None, count,
                                            starts.ctypes.data if count else None, dist.ctypes.data if count else None,
                                            words.ctypes.data if ops and count else None)
    if rc != 0:
        raise _err("%s rc=%d" % (name, rc))
    return starts, dist, words


def palign_edit(P, ptext, k, ends, off=0, n=None, ops=True):
    """(starts, distances, ops) of the END positions `ends` (as pfind_edit returns them for the same P, k, off, n; any order,
    duplicates allowed, any e of the range) — smartgpu_palign_edit64: starts[i] is the LARGEST s with ed(P, T[s..ends[i]]) =
    D(ends[i]) (uint64), distances[i] = D(ends[i]) (uint8, computed), ops the alignment as uint64 of shape (count, 3), two
    bits per operation (edit_cigar reads a row), or None with ops=False (no traceback).  An end with D(e) > k:
    start 2**64 - 1, distance 255, ops 0."""
    return _palign("palign_edit64", P, ptext, k, ends, off, n, ops)


def palign_sets_edit(sets, ptext, k, ends, off=0, n=None, ops=True):
    """palign_edit for a SET pattern (psearch_sets_edit; smartgpu_palign_sets_edit64)."""
    return _palign("palign_sets_edit64", sets, ptext, k, ends, off, n, ops)


def _pfind_then_align(name, find, align, pat, ptext, k, off, n, cap):
    ends, dist, count = find(pat, ptext, k, off=off, n=n, cap=cap)
    if ends is None:
        return None, None, None, None, count
    starts, adist, ops = align(pat, ptext, k, ends, off=off, n=n)
    if not np.array_equal(adist, dist):
        raise SmartGpuError("%s: the align call's distances differ from the find's" % name)
    return starts, ends, dist, ops, count


def pfind_edit_align(P, ptext, k, off=0, n=None, cap=1 << 20):
    """(starts, ends, distances, ops, count): pfind_edit, then palign_edit on its ends — every occurrence of P within edit
    distance k as the interval [start, end] of the text, its distance and its alignment.  More than `cap` occurrences:
    (None, None, None, None, count)."""
    return _pfind_then_align("pfind_edit_align", pfind_edit, palign_edit, P, ptext, k, off, n, cap)


def palign_editl(P, ptext, k, ends, off=0, n=None, ops=True):
    """palign_edit for LONG patterns (psearch_editl: up to 256 symbols, k up to 31; smartgpu_palign_editl64): (starts,
    distances, ops) of the END positions `ends` as pfind_editl returns them — the same contract, with ops as uint64 of shape
    (count, 10) as align_editl returns them: operation t in bits 2 * (t % 32) of word t // 32, words 0 .. 8, the length in
    word 9 (edit_cigar reads a row), or None with ops=False.  An end with D(e) > k: start 2**64 - 1, distance 255, ops 0."""
    return _palign("palign_editl64", P, ptext, k, ends, off, n, ops, ALIGNL_OPS_WORDS)


def palign_sets_editl(sets, ptext, k, ends, off=0, n=None, ops=True):
    """palign_editl for a SET pattern (psearch_sets_editl; smartgpu_palign_sets_editl64)."""
    return _palign("palign_sets_editl64", sets, ptext, k, ends, off, n, ops, ALIGNL_OPS_WORDS)


def pfind_editl_align(P, ptext, k, off=0, n=None, cap=1 << 20):
    """(starts, ends, distances, ops, count): pfind_editl, then palign_editl on its ends — pfind_edit_align for LONG patterns,
    ops of shape (count, 10).  More than `cap` occurrences: (None, None, None, None, count)."""
    return _pfind_then_align("pfind_editl_align", pfind_editl, palign_editl, P, ptext, k, off, n, cap)


def pfind_sets_editl_align(sets, ptext, k, off=0, n=None, cap=1 << 20):
    """pfind_editl_align for a SET pattern (pfind_sets_editl, then palign_sets_editl)."""
    return _pfind_then_align("pfind_sets_editl_align", pfind_sets_editl, palign_sets_editl, sets, ptext, k, off, n, cap)


def edit_cigar(ops_row, sam=False):
    """The run-length string of one alignment (a row of palign_edit's ops: three uint64, the length in the top byte of the
    third; or a row of align_editl's: ten uint64, the length in the tenth), e.g. "12=1X3=1D4=": '=' accepted,
    'X' substituted, 'I' a text symbol with no pattern partner, 'D' a pattern symbol with no text partner — the PATTERN's
    edits.  sam=True swaps the letters I and D: SAM's CIGAR with the text as the reference.  No operations: ""."""
    w = [int(x) for x in ops_row]
    if len(w) not in (3, 10):
        raise ValueError("an alignment is three uint64 words (ten for a long pattern), not %d" % len(w))
    length = w[2] >> 56 if len(w) == 3 else w[9]
    if len(w) == 10 and length > 32 * 9:
        raise ValueError("a long alignment has at most %d operations, not %d" % (32 * 9, length))
    letters = "=XDI" if sam else "=XID"
    out, run, last = [], 0, None
    for t in range(length):
        op = letters[w[t // 32] >> (2 * (t % 32)) & 3]
        if op != last and run:
            out.append("%d%s" % (run, last))
            run = 0
        last = op
        run += 1
    if run:
        out.append("%d%s" % (run, last))
    return "".join(out)


def iupac_revcomp(pattern):
    """The reverse complement of an IUPAC nucleotide pattern (the letters iupac_sets accepts, case preserved, U read as T):
    str for a str, bytes otherwise (smartgpu_iupac_revcomp).  No device needed."""
    is_str = isinstance(pattern, str)
    P = _u8(pattern.encode() if is_str else pattern)
    out = np.zeros(len(P), dtype=np.uint8)
    if lib().smartgpu_iupac_revcomp(P.ctypes.data, len(P), out.ctypes.data) != 0:
        raise _err("iupac_revcomp")
    return out.tobytes().decode() if is_str else out.tobytes()


def iupac_sets(pattern, values, wide=False):
    """The uint8 sets of an IUPAC nucleotide pattern (A C G T U R Y S W K M B D H V N, either case) over a packed text's
    `values` (PackedText.symbols()): bit c of sets[j] = position j accepts values[c].  No device needed.
    At most four values; with wide=True up to eight, the values of a three-plane text (smartgpu_iupac_sets8).  A value that
    is no base letter — N, a separator — is accepted by no letter, pattern letter N included."""
    if isinstance(pattern, str):
        pattern = pattern.encode()
    P = _u8(pattern)
    vals = np.zeros(8, dtype=np.uint8)
    k = len(values)
    vals[:min(k, 8)] = np.asarray(list(values)[:8], dtype=np.uint8)
    sets = np.zeros(len(P), dtype=np.uint8)
    # more than four values: a three-plane text's (smartgpu_iupac_sets8); with at most four, or without `wide`, the call is
    # smartgpu_iupac_sets as ever, refusals included
    call = lib().smartgpu_iupac_sets8 if wide and k > 4 else lib().smartgpu_iupac_sets
    if call(vals.ctypes.data, k, P.ctypes.data, len(P), sets.ctypes.data) != 0:
        raise _err("iupac_sets")
    return sets


def _pattern_set(patterns):
    """K patterns of one length as the const uint8_t* const* the batch calls take (+ what must stay alive)."""
    pats = [_u8(p) for p in patterns]
    m = len(pats[0])
    if any(len(p) != m for p in pats):
        raise SmartGpuError("a pattern set holds patterns of ONE length (smart.c:312 loops per length)")
    ptrs = (C.c_void_p * len(pats))(*[p.ctypes.data for p in pats])
    return pats, ptrs, m


def search_batch(algo, patterns, text, off=0, n=None, per_pattern_times=True, each=False):
    """(counts, pre_ms, run_ms, batch_ms) of `algo` for a whole pattern set over text[off..off+n): the
    harness loop of smart.c:312-345 as one call (smartgpu_search_batch64).  run_ms is None without
    per_pattern_times.  each: every pattern its own launch and event pair (smartgpu_search_batch64_each)."""
    pats, ptrs, m = _pattern_set(patterns)
    K = len(pats)
    if n is None:
        n = len(text) - off
    counts = np.zeros(K, dtype=np.uint64)
    pre = np.zeros(K, dtype=np.float64)
    run = np.zeros(K, dtype=np.float64) if per_pattern_times else None
    batch = C.c_double(0.0)
    fn = lib().smartgpu_search_batch64_each if each else lib().smartgpu_search_batch64
    rc = fn(algo_id(algo), C.cast(ptrs, C.c_void_p), m, K, text._h, off, n, counts.ctypes.data,
            pre.ctypes.data, run.ctypes.data if run is not None else None, C.byref(batch))
    if rc != 0:
        raise _err("search_batch64(%s) rc=%d" % (algo, rc))
    return counts, pre, run, float(batch.value)


def find(P, text, off=0, n=None, cap=1 << 20):
    """(positions, count): the ascending start offsets (relative to text byte 0) of P in
    text[off..off+n), and their number.  When there are more than `cap`, positions is None and only
    the count is returned (smartgpu_find64 reports SMARTGPU_ERR_NOMEM; retry with cap >= count)."""
    P = _u8(P)
    if n is None:
        n = len(text) - off
    out = np.empty(max(cap, 1), dtype=np.uint64)
    c = C.c_uint64(0)
    rc = lib().smartgpu_find64(P.ctypes.data, len(P), text._h, off, n, out.ctypes.data, cap, C.byref(c))
    if rc == -5 and c.value > cap:
        return None, int(c.value)
    if rc != 0:
        raise _err("find64 rc=%d" % rc)
    return out[:c.value].copy(), int(c.value)


FIND_BATCH_MAX_K = 1 << 18          # multi_find.hpp: kFindBatchMaxK
FIND_BATCH_STAGING = 32 << 20       # include/smartgpu.h: SMARTGPU_FIND_BATCH_STAGING


def find_width(m):
    """Patterns of length m that one pass of hor_multi_find decides (multi_find.hpp: find_width): what the LDS of a
    workgroup holds beside the table, the stage and the tile when four are resident on a CU."""
    stride = (min(m, 65) + 15) // 16 * 16
    return {16: 208, 32: 124, 48: 89, 64: 69, 80: 56}[stride]


def find_batch_max(m):
    """The most patterns of length m that one smartgpu_find_batch64 call takes (multi_find.hpp: find_batch_max)."""
    stride = (min(m, 65) + 15) // 16 * 16
    staged = stride + ((m + 15) // 16 * 16 if m - 1 > 16 else 0)
    return min(FIND_BATCH_STAGING // staged, FIND_BATCH_MAX_K)


def _find_batch_one(pats, text, off, n, cap):
    """One smartgpu_find_batch64 call: (list of len(pats) ascending uint64 arrays or None, counts) for patterns of ONE
    length; None when their occurrences are more than `cap`."""
    pats, ptrs, m = _pattern_set(pats)
    K = len(pats)
    out = np.empty(max(cap, 1), dtype=np.uint64)
    starts = np.zeros(K + 1, dtype=np.uint64)
    rc = lib().smartgpu_find_batch64(C.cast(ptrs, C.c_void_p), m, K, text._h, off, n, out.ctypes.data if cap else None, cap,
                                     starts.ctypes.data)
    counts = np.diff(starts)
    if rc == -5 and int(starts[K]) > cap:
        return None, counts
    if rc != 0:
        raise _err("find_batch64 rc=%d" % rc)
    return [out[int(starts[k]):int(starts[k + 1])].copy() for k in range(K)], counts


def find_batch(patterns, text, off=0, n=None, cap=1 << 20):
    """(list of K ascending uint64 arrays, counts): the start offsets (relative to text byte 0) of every pattern of a set
    in text[off..off+n), found in shared passes over the text (smartgpu_find_batch64), and their numbers, in the caller's
    order.  `cap` is the room for the positions of ALL patterns; when they are more, the list is None and the counts say
    how much room a retry needs.  Patterns of several lengths are grouped by length, one call per length."""
    pats = [_u8(p) for p in patterns]
    if not pats:
        raise SmartGpuError("find_batch: an empty pattern set")
    if n is None:
        n = len(text) - off
    by_len = {}
    for i, p in enumerate(pats):
        by_len.setdefault(len(p), []).append(i)
    lists = [None] * len(pats)
    counts = np.zeros(len(pats), dtype=np.uint64)
    left = cap  # None: the room is used up, the remaining lengths only count
    for m in sorted(by_len):
        idx = by_len[m]
        got, c = _find_batch_one([pats[i] for i in idx], text, off, n, left if left is not None else 0)
        counts[idx] = c
        if left is not None and got is not None:
            for i, g in zip(idx, got):
                lists[i] = g
            left -= int(c.sum())
        else:
            left = None
    if left is None and int(counts.sum()) > cap:
        return None, counts
    return lists, counts


def _classes(classes):
    """An (m, 32) uint8 array of 256-bit rows (byte_classes) as the calls take it, and m."""
    classes = np.ascontiguousarray(classes, dtype=np.uint8)
    if classes.ndim != 2 or classes.shape[1] != 32:
        raise ValueError("classes: an (m, 32) uint8 array, one 256-bit row per pattern position, not shape %r" % (classes.shape,))
    return classes, classes.shape[0]


def byte_classes(P, ignore_case=False):
    """The (len(P), 32) uint8 array search_edit_classes / find_edit_classes take, from a byte pattern: row j bit v (byte v // 8,
    bit v % 8) set means position j accepts byte value v.  Every row holds the one bit of P[j]; with ignore_case a letter's
    row holds both of its cases (ASCII folding only: A-Z and a-z, nothing beyond 127)."""
    P = _u8(P)
    rows = np.zeros((len(P), 32), dtype=np.uint8)
    for j, v in enumerate(P.tolist()):
        rows[j, v >> 3] |= 1 << (v & 7)
        if ignore_case and (65 <= v <= 90 or 97 <= v <= 122):
            w = v ^ 0x20
            rows[j, w >> 3] |= 1 << (w & 7)
    return rows


def _tedit_count(name, pat, m, text, k, off, n, *flags):
    if n is None:
        n = len(text) - off
    c = C.c_uint64(0)
    rc = getattr(lib(), "smartgpu_" + name)(pat.ctypes.data, m, k, *flags, text._h, off, n, C.byref(c), None, None)
    if rc != 0:
        raise _err("%s rc=%d" % (name, rc))
    return int(c.value)


def _tedit_find(name, pat, m, text, k, off, n, cap, *flags):
    if n is None:
        n = len(text) - off
    ends = np.empty(max(cap, 1), dtype=np.uint64)
    dist = np.empty(max(cap, 1), dtype=np.uint8)
    c = C.c_uint64(0)
    rc = getattr(lib(), "smartgpu_" + name)(pat.ctypes.data, m, k, *flags, text._h, off, n, ends.ctypes.data if cap else None,
                                            dist.ctypes.data if cap else None, cap, C.byref(c))
    if rc != 0:  # (more than cap occurrences: SMARTGPU_ERR_NOMEM, the message holds the count a retry needs)
        raise _err("%s rc=%d" % (name, rc))
    return ends[:c.value].copy(), dist[:c.value].copy()


def search_edit(P, text, k, off=0, n=None):
    """The number of END positions e in bytes [off, off+n) of a Text where P occurs within edit distance k — substitutions,
    insertions and deletions, 0 <= k <= 7, 1 <= len(P) <= 64 (smartgpu_search_edit64): some substring [s, e] of the range,
    off <= s, is at most k edits from P.  The text may hold any byte values."""
    P = _u8(P)
    return _tedit_count("search_edit64", P, len(P), text, k, off, n)


def find_edit(P, text, k, off=0, n=None, cap=1 << 20):
    """(ends, distances) of P within edit distance k (search_edit) in bytes [off, off+n) of a Text: the ascending end
    positions (uint64, the match's last byte, relative to text byte 0) and the edit distance of each (uint8).  More than
    `cap` occurrences raise SmartGpuError; its text names their number (smartgpu_find_edit64)."""
    P = _u8(P)
    return _tedit_find("find_edit64", P, len(P), text, k, off, n, cap)


def search_edit_classes(classes, text, k, off=0, n=None):
    """search_edit for a pattern of byte CLASSES: an (m, 32) uint8 array whose row j says which byte values position j
    accepts (byte_classes; smartgpu_search_edit_classes64).  An empty row accepts nothing, a full row everything."""
    classes, m = _classes(classes)
    return _tedit_count("search_edit_classes64", classes, m, text, k, off, n)


def find_edit_classes(classes, text, k, off=0, n=None, cap=1 << 20):
    """(ends, distances) of a pattern of byte classes (search_edit_classes), as find_edit returns them."""
    classes, m = _classes(classes)
    return _tedit_find("find_edit_classes64", classes, m, text, k, off, n, cap)


def search_editl(P, text, k, off=0, n=None, all_blocks=False):
    """search_edit for LONG patterns: 1 <= len(P) <= 256, 0 <= k <= 31 (smartgpu_search_editl64; Myers' recurrence in blocks of
    32 rows with Ukkonen's cut-off).  The same contract, and for len(P) <= 64, k <= 7 the same answers.  all_blocks=True
    computes every block of every column (SMARTGPU_EDITL_ALL_BLOCKS): the same answers, for cross-checks and measurements."""
    P = _u8(P)
    return _tedit_count("search_editl64", P, len(P), text, k, off, n, int(bool(all_blocks)))


def find_editl(P, text, k, off=0, n=None, cap=1 << 20, all_blocks=False):
    """(ends, distances) as find_edit returns them, for LONG patterns (search_editl; smartgpu_find_editl64)."""
    P = _u8(P)
    return _tedit_find("find_editl64", P, len(P), text, k, off, n, cap, int(bool(all_blocks)))


def search_editl_classes(classes, text, k, off=0, n=None, all_blocks=False):
    """search_editl for a pattern of byte CLASSES (search_edit_classes' rows; smartgpu_search_editl_classes64)."""
    classes, m = _classes(classes)
    return _tedit_count("search_editl_classes64", classes, m, text, k, off, n, int(bool(all_blocks)))


def find_editl_classes(classes, text, k, off=0, n=None, cap=1 << 20, all_blocks=False):
    """(ends, distances) of a pattern of byte classes, for LONG patterns (smartgpu_find_editl_classes64)."""
    classes, m = _classes(classes)
    return _tedit_find("find_editl_classes64", classes, m, text, k, off, n, cap, int(bool(all_blocks)))


def search_mis(P, text, k, off=0, n=None):
    """The number of START positions s, off <= s <= off + n - len(P), in bytes [off, off+n) of a Text whose window of len(P)
    bytes differs from P in at most k positions — substitutions only, no shifts; 0 <= k <= 7, 1 <= len(P) <= 64
    (smartgpu_search_mis64).  The text may hold any byte values; a byte of P it does not hold is a mismatch in every window."""
    P = _u8(P)
    return _tedit_count("search_mis64", P, len(P), text, k, off, n)


def find_mis(P, text, k, off=0, n=None, cap=1 << 20):
    """(positions, mismatches) of P with at most k mismatches (search_mis) in bytes [off, off+n) of a Text: the ascending start
    positions (uint64, relative to text byte 0) and the number of mismatches of each (uint8).  More than `cap` occurrences
    raise SmartGpuError; its text names their number (smartgpu_find_mis64)."""
    P = _u8(P)
    return _tedit_find("find_mis64", P, len(P), text, k, off, n, cap)


def search_mis_classes(classes, text, k, off=0, n=None):
    """search_mis for a pattern of byte CLASSES: an (m, 32) uint8 array whose row j says which byte values position j accepts
    (byte_classes; smartgpu_search_mis_classes64).  An empty row is a mismatch in every window, a full row never is."""
    classes, m = _classes(classes)
    return _tedit_count("search_mis_classes64", classes, m, text, k, off, n)


def find_mis_classes(classes, text, k, off=0, n=None, cap=1 << 20):
    """(positions, mismatches) of a pattern of byte classes (search_mis_classes), as find_mis returns them."""
    classes, m = _classes(classes)
    return _tedit_find("find_mis_classes64", classes, m, text, k, off, n, cap)


def _talign(name, pat, m, text, k, ends, off, n, ops, words_per=3):
    if n is None:
        n = len(text) - off
    ends = np.ascontiguousarray(ends, dtype=np.uint64)
    count = len(ends)
    starts = np.empty(count, dtype=np.uint64)
    dist = np.empty(count, dtype=np.uint8)
    words = np.empty((count, words_per), dtype=np.uint64) if ops else None
    rc = getattr(lib(), "smartgpu_" + name)(pat.ctypes.data, m, k, text._h, off, n, ends.ctypes.data if count else None, count,
                                            starts.ctypes.data if count else None, dist.ctypes.data if count else None,
                                            words.ctypes.data if ops and count else None)
    if rc != 0:
        raise _err("%s rc=%d" % (name, rc))
    return starts, dist, words


def align_edit(P, text, k, ends, off=0, n=None, ops=True):
    """(starts, distances, ops) of the END positions `ends` on a Text (as find_edit returns them for the same P, k, off, n; any
    order, duplicates allowed, any e of the range) — smartgpu_align_edit64, palign_edit's contract on bytes: starts[i] is the
    LARGEST s with ed(P, T[s..ends[i]]) = D(ends[i]) (uint64), distances[i] = D(ends[i]) (uint8, computed), ops the alignment
    as uint64 of shape (count, 3) (edit_cigar reads a row), or None with ops=False (no traceback).  An end with D(e) > k:
    start 2**64 - 1, distance 255, ops 0."""
    P = _u8(P)
    return _talign("align_edit64", P, len(P), text, k, ends, off, n, ops)


def align_edit_classes(classes, text, k, ends, off=0, n=None, ops=True):
    """align_edit for a pattern of byte CLASSES (search_edit_classes; smartgpu_align_edit_classes64)."""
    classes, m = _classes(classes)
    return _talign("align_edit_classes64", classes, m, text, k, ends, off, n, ops)


def _find_then_align(name, find, align, pat, text, k, off, n, cap):
    ends, dist = find(pat, text, k, off=off, n=n, cap=cap)
    starts, adist, ops = align(pat, text, k, ends, off=off, n=n)
    if not np.array_equal(adist, dist):
        raise SmartGpuError("%s: the align call's distances differ from the find's" % name)
    return starts, ends, dist, ops


def find_edit_align(P, text, k, off=0, n=None, cap=1 << 20):
    """(starts, ends, distances, ops): find_edit, then align_edit on its ends — every occurrence of P within edit distance k as
    the interval [start, end] of the text, its distance and its alignment.  More than `cap` occurrences raise SmartGpuError,
    as find_edit does."""
    return _find_then_align("find_edit_align", find_edit, align_edit, P, text, k, off, n, cap)


def find_edit_classes_align(classes, text, k, off=0, n=None, cap=1 << 20):
    """find_edit_align for a pattern of byte classes (find_edit_classes, then align_edit_classes)."""
    return _find_then_align("find_edit_classes_align", find_edit_classes, align_edit_classes, classes, text, k, off, n, cap)


ALIGNL_OPS_WORDS = 10  # SMARTGPU_ALIGNL_OPS_WORDS


def align_editl(P, text, k, ends, off=0, n=None, ops=True):
    """align_edit for LONG patterns (search_editl: up to 256 bytes, k up to 31; smartgpu_align_editl64): (starts, distances,
    ops) of the END positions `ends` as find_editl returns them — the same contract, with ops as uint64 of shape (count, 10):
    operation t in bits 2 * (t % 32) of word t // 32, words 0 .. 8, the length in word 9 (edit_cigar reads a row), or None
    with ops=False.  An end with D(e) > k: start 2**64 - 1, distance 255, ops 0."""
    P = _u8(P)
    return _talign("align_editl64", P, len(P), text, k, ends, off, n, ops, ALIGNL_OPS_WORDS)


def align_editl_classes(classes, text, k, ends, off=0, n=None, ops=True):
    """align_editl for a pattern of byte CLASSES (search_editl_classes; smartgpu_align_editl_classes64)."""
    classes, m = _classes(classes)
    return _talign("align_editl_classes64", classes, m, text, k, ends, off, n, ops, ALIGNL_OPS_WORDS)


def find_editl_align(P, text, k, off=0, n=None, cap=1 << 20):
    """(starts, ends, distances, ops): find_editl, then align_editl on its ends — find_edit_align for LONG patterns, ops of
    shape (count, 10)."""
    return _find_then_align("find_editl_align", find_editl, align_editl, P, text, k, off, n, cap)


def find_editl_classes_align(classes, text, k, off=0, n=None, cap=1 << 20):
    """find_editl_align for a pattern of byte classes (find_editl_classes, then align_editl_classes)."""
    return _find_then_align("find_editl_classes_align", find_editl_classes, align_editl_classes, classes, text, k, off, n, cap)


def search_host(algo, P, T):
    """SMART's own `int search(P, m, T, n)` shape on host buffers."""
    P = _u8(P)
    T = _u8(T)
    return getattr(lib(), "smartgpu_%s_search" % algo)(P.ctypes.data, len(P), T.ctypes.data, len(T))


def device_sync(device=0):
    if lib().smartgpu_device_sync(device) != 0:
        raise _err("device_sync")


def stream_mark(device, which):
    if lib().smartgpu_stream_mark(device, which) != 0:
        raise _err("stream_mark")


def stream_elapsed_ms(device):
    ms = C.c_double(0.0)
    if lib().smartgpu_stream_elapsed_ms(device, C.byref(ms)) != 0:
        raise _err("stream_elapsed_ms")
    return float(ms.value)


def probe_read_gbs(text, reps=20):
    """Practical streaming-read rate (GB/s) of the device on this text."""
    ms = C.c_double(0.0)
    if lib().smartgpu_probe_read_ms(text._h, reps, C.byref(ms)) != 0:
        raise _err("probe_read")
    return len(text) / (ms.value * 1e-3) / 1e9


def tune(key, value):
    if lib().smartgpu_tune(key, value) != 0:
        raise _err("tune")


def coalesce(max_group):
    """How many queued Plan.launch calls share one pass over the text (0: none, 2..8); returns the previous value,
    a wider one (coalesce_wide) as 8."""
    prev = lib().smartgpu_coalesce(max_group)
    if prev < 0:
        raise _err("coalesce")
    return prev


def coalesce_wide(max_group):
    """coalesce() up to 32 (0: none, 2..32); returns the previous value, a wider one (coalesce_pass) as 32."""
    prev = lib().smartgpu_coalesce_wide(max_group)
    if prev < 0:
        raise _err("coalesce")
    return prev


PASS_MAX = 96


def pass_width(m):
    """The most patterns of length m one pass takes: two pointers and the pattern's last min(m, 65) bytes, rounded
    to 16, for each of them in 4032 bytes of kernel arguments (smart_amd/csrc/multi.hpp: pass_width)."""
    return min(PASS_MAX, 4032 // (16 + (min(m, 65) + 15) // 16 * 16))


def coalesce_pass(max_group):
    """coalesce() over the setting's whole range (0: none, 2..96; clipped per pattern length to pass_width(m));
    returns the previous value as it was."""
    prev = lib().smartgpu_coalesce_pass(max_group)
    if prev < 0:
        raise _err("coalesce")
    return prev


LONG_DEFAULT = 64 << 20


def long_width(m):
    """The most patterns of length m a LONG pass takes (smart_amd/csrc/multi.hpp: long_width): such a pass carries two
    pointers per pattern in the 4032 bytes and reads the rows from the plans, so what bounds it is a thread per pattern
    (252) and the LDS of a workgroup at four per CU: 40960 bytes for the table (16384), the heads (2048), a link and a
    sum per pattern, the rows rounded to 64, and the tile (16448)."""
    stride = (min(m, 65) + 15) // 16 * 16
    np = 0
    while 16 * (np + 1) <= 4032 and np + 1 <= 256 - 4 and 16384 + 2048 + 8 * (np + 1) + (((np + 1) * stride + 63) & ~63) + 16448 <= 40960:
        np += 1
    return np


def coalesce_long(min_range_bytes):
    """The least range, in bytes, over which a key whose previous pass left full goes on gathering beyond pass_width(m),
    up to long_width(m) (-1: never, 0: any range; the library starts with LONG_DEFAULT); returns the previous value.
    A key whose launches arrive faster than the GPU could use an early pass gathers on in the same way (api.cpp, rule (c))."""
    prev = lib().smartgpu_coalesce_long(min_range_bytes)
    if prev < -1:
        raise _err("coalesce_long")
    return prev


def coalesce_stats(device=0):
    """(launches that could share a pass, kernels sent for them) on `device` so far."""
    launches, passes = C.c_uint64(0), C.c_uint64(0)
    if lib().smartgpu_coalesce_stats(device, C.byref(launches), C.byref(passes)) != 0:
        raise _err("coalesce_stats")
    return int(launches.value), int(passes.value)


def coalesce_riders(device=0):
    """Launches on `device` so far that rode in a pass gathering beside them: patterns whose own symbols repeat, over a
    text whose symbols do not (Text.repeat_rate() at most 1/48).  They are not among coalesce_stats()' launches."""
    riders = C.c_uint64(0)
    if lib().smartgpu_coalesce_riders(device, C.byref(riders)) != 0:
        raise _err("coalesce_riders")
    return int(riders.value)


SAMPLING_DEFAULT = 64 << 20
SAMPLE_STRIDE, SAMPLE_GRAM, SAMPLE_MIN_M = 28, 4, 31
SAMPLE_WIDTH, SAMPLE_LONG_WIDTH = 84, 252


def text_sampling(min_bytes):
    """The least text, in bytes, that gets a sample when it is created — the 4 bytes at every 28th position, n / 7 bytes
    (-1: none, 0: every text; the library starts with SAMPLING_DEFAULT); returns the previous value."""
    prev = lib().smartgpu_text_sampling(min_bytes)
    if prev < -1:
        raise _err("text_sampling")
    return prev


def text_has_sample(text):
    """Does this Text carry a sample?"""
    return bool(lib().smartgpu_text_has_sample(text._h))


def coalesce_sample(on):
    """Shared passes of patterns of 31 bytes or more over a text that has a sample read the sample, not the text
    (hor_sample_scan); False sends them to hor_multi_scan as before.  Returns the previous setting."""
    return bool(lib().smartgpu_coalesce_sample(1 if on else 0))


def coalesce_sampled(device=0):
    """Passes on `device` so far that went to hor_sample_scan (they are among coalesce_stats()' passes)."""
    passes = C.c_uint64(0)
    if lib().smartgpu_coalesce_sampled(device, C.byref(passes)) != 0:
        raise _err("coalesce_sampled")
    return int(passes.value)


def coalesce_sample_grid(workgroups):
    """The workgroups of a sampled pass (0: one per compute unit); for measurements and tests.  Returns the previous value."""
    prev = lib().smartgpu_coalesce_sample_grid(workgroups)
    if prev < 0:
        raise _err("coalesce_sample_grid")
    return prev


def kernel_for(algo, P):
    """Kernel a plan of (algo, P) would launch under the current tune settings; no device needed."""
    P = _u8(P)
    name = lib().smartgpu_kernel_for(algo_id(algo), P.ctypes.data, len(P))
    if name is None:
        raise _err("kernel_for")
    return name.decode()


def build_table(which, P):
    P = _u8(P)
    names = {"bad_char": 0, "good_suffix": 1, "kmp_next": 2, "shift_or": 3, "bndm": 4, "kmp_dfa": 5,
             "kmp_dfa_compressed": 6, "shift_and": 7, "quick_search": 8, "kmp_runs": 9, "four_codes": 10, "kmp_runs_compact": 11, "hash3": 13, "hash5": 15, "hash8": 18}
    out = np.empty(max(257, len(P) + 1, (len(P) + 1) * 256 + 257 if which.startswith("kmp_dfa") else 256 * 256 + 272 if which.startswith("kmp_runs") else 0), dtype=np.int32)
    k = lib().smartgpu_build_table(names[which], P.ctypes.data, len(P), out.ctypes.data, len(out))
    if k < 0:
        raise _err("build_table")
    return out[:k].copy()
