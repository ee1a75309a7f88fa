"""ctypes binding of libmfa_hip.so (include/mfa_hip.h).

Thin by design: the product is the C-ABI library; Python is used by the tests and the
bench to allocate device memory (torch) and to launch ranks (torch.distributed).
There is no fallback: if the library is missing, loading raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MFA_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "csrc", "libmfa_hip.so")      # (the override: development builds)

OK = 0
KERNEL_NONE, KERNEL_WALK, KERNEL_SPECIALISED, KERNEL_TABLE, KERNEL_NODESET, KERNEL_SEARCH = 0, 1, 2, 3, 4, 5
ERR_INVALID_ARG, ERR_BAD_BLOB, ERR_UNSUPPORTED, ERR_NO_DEVICE, ERR_HIP, ERR_NOMEM, ERR_TOO_LONG, ERR_JIT = -1, -2, -3, -4, -5, -6, -7, -8

EXPORTS = ["mfa_image_create", "mfa_image_destroy", "mfa_image_get_info", "mfa_image_prepare", "mfa_image_specialize", "mfa_match_batch",
           "mfa_match_batch_regions", "mfa_region_scan", "mfa_match_batch_host", "mfa_last_kernel_ms", "mfa_last_region_ms",
           "mfa_device_count", "mfa_last_hip_error", "mfa_strerror", "mfa_version",
           "mfa_mixed_create", "mfa_mixed_destroy", "mfa_match_mixed", "mfa_match_mixed_sized", "mfa_match_mixed_host", "mfa_mixed_last_ms", "mfa_mixed_timing",
           "mfa_mixed_last_launches", "mfa_mixed_last_dfa", "mfa_pack_result_bitmap", "mfa_last_dfa_split",
           "mfa_match_batch_resume", "mfa_match_batch_resume_host", "mfa_last_dfa_spec",
           "mfa_match_batch_resume_set", "mfa_match_batch_resume_set_host", "mfa_last_set_split",
           "mfa_match_batch_resume_set_wide", "mfa_match_batch_resume_set_wide_host", "mfa_image_resume_state_bytes",
           "mfa_split_tile_bytes", "mfa_split_workspace_bytes", "mfa_split_text_count", "mfa_split_text_write",
           "mfa_select_workspace_bytes", "mfa_select_count", "mfa_select_write",
           "mfa_search_batch", "mfa_search_batch_host", "mfa_image_search_info"]

DFA_STATE_DEAD, DFA_STATE_START, DFA_STATE_INVALID = 0, 1, 0xffffffff      # words of mfa_match_batch_resume (never stored)
SET_STATE_WORDS = 12                                                        # a record of mfa_match_batch_resume_set: tag, reserved[3], nodes[8]
SET_STATE_WIDE_WORDS = 68                                                   # a record of mfa_match_batch_resume_set_wide (wave images): tag, reserved[3], nodes[64]
SET_STATE_START, SET_STATE_LIVE, SET_STATE_INVALID = 0, 1, 0xffffffff       # their tags (records are never stored either)
REGION_WORDS, REGION_MAX, REGION_OVERFLOW, REGION_MIN_LEN = 16, 15, 0x100, 64
SPLIT_LINES, SPLIT_TOKENS = 0, 1                                            # modes of the text splitter
SELECT_INVERT, SELECT_NEWLINE = 1, 2                                        # flags of the selection


class MfaError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        msg = lib().mfa_strerror(code).decode()
        if code == ERR_HIP:
            msg += " (hipError %d)" % lib().mfa_last_hip_error()
        super().__init__("%s: %s [%d]" % (where, msg, code))


class ImageInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in
                ("kind", "is_reversed", "n_nodes", "n_edges", "n_cells", "dfa_states", "byte_classes", "last_kernel")]


class SplitInfo(ctypes.Structure):
    """mfa_split_info: 32 bytes of device memory"""
    _fields_ = [("n_strings", ctypes.c_uint64), ("n_bytes", ctypes.c_uint64), ("max_string_bytes", ctypes.c_uint64),
                ("stopped", ctypes.c_uint32), ("overflow", ctypes.c_uint32)]


class SelectInfo(ctypes.Structure):
    """mfa_select_info: 32 bytes of device memory"""
    _fields_ = [("n_selected", ctypes.c_uint64), ("n_bytes", ctypes.c_uint64), ("n_unanswered", ctypes.c_uint64),
                ("overflow", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libmfa_hip.so is not built (run python -c 'import __graft_entry__ as g; g.build()'): "
                              + LIB_PATH)
        # A process must hold ONE HIP runtime.  torch bundles its own libamdhip64 (same soname as
        # /opt/rocm's): load torch first so the dynamic loader resolves our NEEDED entry to the copy
        # torch already mapped instead of mapping a second runtime that cannot see the device.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
        L.mfa_image_create.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(vp)]
        L.mfa_image_create.restype = i32
        L.mfa_image_destroy.argtypes = [vp]
        L.mfa_image_destroy.restype = None
        L.mfa_image_get_info.argtypes = [vp, ctypes.POINTER(ImageInfo)]
        L.mfa_image_prepare.argtypes = [vp, i32]
        L.mfa_image_specialize.argtypes = [vp]
        L.mfa_match_batch.argtypes = [vp, vp, vp, u64, vp, i32, vp]
        L.mfa_match_batch_regions.argtypes = [vp, vp, vp, u64, vp, vp, i32, vp]
        L.mfa_region_scan.argtypes = [vp, vp, u64, vp, i32, vp]
        L.mfa_last_region_ms.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_float)]
        L.mfa_match_batch_host.argtypes = [vp, vp, vp, u64, vp, i32]
        L.mfa_match_batch_resume.argtypes = [vp, vp, vp, u64, vp, vp, i32, vp]
        L.mfa_match_batch_resume_host.argtypes = [vp, vp, vp, u64, vp, vp, i32]
        if hasattr(L, "mfa_match_batch_resume_set"):      # (a library of an older build given by MFA_LIB_PATH for an A/B run lacks it)
            L.mfa_match_batch_resume_set.argtypes = [vp, vp, vp, u64, vp, vp, i32, vp]
            L.mfa_match_batch_resume_set_host.argtypes = [vp, vp, vp, u64, vp, vp, i32]
        if hasattr(L, "mfa_match_batch_resume_set_wide"):      # (as above: an older build)
            L.mfa_match_batch_resume_set_wide.argtypes = [vp, vp, vp, u64, vp, vp, i32, vp]
            L.mfa_match_batch_resume_set_wide_host.argtypes = [vp, vp, vp, u64, vp, vp, i32]
            L.mfa_image_resume_state_bytes.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32)]
        L.mfa_last_kernel_ms.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_float)]
        if hasattr(L, "mfa_last_dfa_split"):              # (a library of an older build given by MFA_LIB_PATH for an A/B run lacks it)
            L.mfa_last_dfa_split.argtypes = [vp, i32, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_uint32)]
        if hasattr(L, "mfa_last_dfa_spec"):               # (as above: an older build)
            L.mfa_last_dfa_spec.argtypes = [vp, i32, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]
        if hasattr(L, "mfa_last_set_split"):              # (as above: an older build)
            L.mfa_last_set_split.argtypes = [vp, i32, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_uint32)] + [ctypes.POINTER(u64)] * 3
        L.mfa_mixed_create.argtypes = [ctypes.POINTER(vp), ctypes.c_uint32, ctypes.POINTER(vp)]
        L.mfa_mixed_destroy.argtypes = [vp]
        L.mfa_mixed_destroy.restype = None
        L.mfa_match_mixed.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64), vp, i32, vp]
        L.mfa_match_mixed_sized.argtypes = [vp, vp, vp, u64, u64, ctypes.POINTER(u64), vp, i32, vp]
        L.mfa_mixed_last_launches.argtypes = [vp, i32] + [ctypes.POINTER(ctypes.c_uint32)] * 4
        if hasattr(L, "mfa_mixed_last_dfa"):              # (as above: an older build)
            L.mfa_mixed_last_dfa.argtypes = [vp, i32] + [ctypes.POINTER(ctypes.c_uint32)] * 3 + [ctypes.POINTER(u64)]
        L.mfa_pack_result_bitmap.argtypes = [vp, u64, vp, vp]
        L.mfa_match_mixed_host.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64), vp, i32]
        L.mfa_mixed_last_ms.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
        L.mfa_mixed_timing.argtypes = [vp, i32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
        if hasattr(L, "mfa_split_text_count"):            # (as above: an older build)
            L.mfa_split_tile_bytes.restype = ctypes.c_uint32
            L.mfa_split_workspace_bytes.argtypes = [u64, ctypes.POINTER(ctypes.c_size_t)]
            L.mfa_split_text_count.argtypes = [vp, u64, ctypes.c_uint32, ctypes.c_char_p, vp, vp, i32, vp]
            L.mfa_split_text_write.argtypes = [vp, u64, ctypes.c_uint32, vp, vp, vp, u64, vp, u64, i32, vp]
        if hasattr(L, "mfa_select_count"):                # (as above: an older build)
            L.mfa_select_workspace_bytes.argtypes = [u64, ctypes.POINTER(ctypes.c_size_t)]
            L.mfa_select_count.argtypes = [vp, vp, u64, ctypes.c_uint32, vp, vp, i32, vp]
            L.mfa_select_write.argtypes = [vp, vp, vp, u64, ctypes.c_uint32, vp, vp, vp, u64, vp, vp, u64, i32, vp]
        if hasattr(L, "mfa_search_batch"):                # (as above: an older build)
            L.mfa_search_batch.argtypes = [vp, vp, vp, u64, vp, vp, vp, i32, vp]
            L.mfa_search_batch_host.argtypes = [vp, vp, vp, u64, vp, vp, vp, i32]
            L.mfa_image_search_info.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        L.mfa_strerror.argtypes = [i32]
        L.mfa_strerror.restype = ctypes.c_char_p
        L.mfa_version.restype = ctypes.c_char_p
        _lib = L
    return _lib


def _check(rc, where):
    if rc != OK:
        raise MfaError(rc, where)


class Image:
    """An automaton image handle (mfa_image_t*)."""

    def __init__(self, blob):
        self._h = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(bytes(blob), len(blob))
        _check(lib().mfa_image_create(buf, len(blob), ctypes.byref(self._h)), "mfa_image_create")

    def info(self):
        out = ImageInfo()
        _check(lib().mfa_image_get_info(self._h, ctypes.byref(out)), "mfa_image_get_info")
        return {n: getattr(out, n) for n, _ in ImageInfo._fields_}

    def specialize(self):
        """Generate and compile the automaton-specific kernel into the on-disk cache (no GPU needed).
        Returns False when the automaton is too large for a specialised kernel."""
        rc = lib().mfa_image_specialize(self._h)
        if rc == ERR_UNSUPPORTED:
            return False
        _check(rc, "mfa_image_specialize")
        return True

    def prepare(self, device=0):
        _check(lib().mfa_image_prepare(self._h, device), "mfa_image_prepare")

    def match_device(self, d_bytes_ptr, d_offsets_ptr, n, d_results_ptr, device=0, stream=0):
        """Raw device pointers (ints); asynchronous on `stream` (a hipStream_t value, 0 = default)."""
        _check(lib().mfa_match_batch(self._h, d_bytes_ptr, d_offsets_ptr, n, d_results_ptr, device,
                                     ctypes.c_void_p(stream)), "mfa_match_batch")

    def match_tensors(self, d_bytes, d_offsets, d_results=None, stream=None):
        """torch CUDA tensors: uint8 bytes, int64 offsets (n+1) -> uint8 results (n).  Enqueued on
        `stream` (torch stream; default: the current one)."""
        import torch
        n = d_offsets.numel() - 1
        dev = d_offsets.device.index or 0
        if d_results is None:
            d_results = torch.empty(max(n, 1), dtype=torch.uint8, device=d_offsets.device)
        s = stream if stream is not None else torch.cuda.current_stream(d_offsets.device)
        self.match_device(d_bytes.data_ptr(), d_offsets.data_ptr(), n, d_results.data_ptr(), dev, s.cuda_stream)
        return d_results[:n]

    def match_tensors_regions(self, d_bytes, d_offsets, d_table, d_results=None, stream=None):
        """mfa_match_batch_regions: like match_tensors, with a region table the caller has filled (region_scan) for
        exactly these strings; d_table None = no table (every step is executed)."""
        import torch
        n = d_offsets.numel() - 1
        dev = d_offsets.device.index or 0
        if d_results is None:
            d_results = torch.empty(max(n, 1), dtype=torch.uint8, device=d_offsets.device)
        s = stream if stream is not None else torch.cuda.current_stream(d_offsets.device)
        _check(lib().mfa_match_batch_regions(self._h, d_bytes.data_ptr(), d_offsets.data_ptr(), n, d_results.data_ptr(),
                                             d_table.data_ptr() if d_table is not None else None, dev,
                                             ctypes.c_void_p(s.cuda_stream)), "mfa_match_batch_regions")
        return d_results[:n]

    def last_region_ms(self, device=0):
        ms = ctypes.c_float()
        _check(lib().mfa_last_region_ms(self._h, device, ctypes.byref(ms)), "mfa_last_region_ms")
        return ms.value

    def match_host(self, data, offsets, device=0):
        """numpy uint8 data + uint64 offsets(n+1) in host memory -> numpy uint8 results."""
        import numpy as np
        n = len(offsets) - 1
        res = np.zeros(max(n, 1), dtype=np.uint8)
        _check(lib().mfa_match_batch_host(self._h, data.ctypes.data, offsets.ctypes.data, n, res.ctypes.data, device),
               "mfa_match_batch_host")
        return res[:n]

    def match_tensors_resume(self, d_bytes, d_offsets, d_states, d_results=None, stream=None):
        """mfa_match_batch_resume on torch CUDA tensors: one round of pieces of n strings, in scan order (a reversed image takes a
        string's LAST piece first).  d_states: int32 or uint32 tensor of n words, updated in place (DFA_STATE_START before a string's first
        piece); d_results: uint8 tensor of n bytes, or None for no result bytes.  Returns d_results.  Asynchronous on `stream`."""
        import torch
        n = d_offsets.numel() - 1
        assert d_states.element_size() == 4 and d_states.numel() >= n
        dev = d_offsets.device.index or 0
        s = stream if stream is not None else torch.cuda.current_stream(d_offsets.device)
        _check(lib().mfa_match_batch_resume(self._h, d_bytes.data_ptr(), d_offsets.data_ptr(), n, d_states.data_ptr(),
                                            d_results.data_ptr() if d_results is not None else None, dev, ctypes.c_void_p(s.cuda_stream)),
               "mfa_match_batch_resume")
        return d_results

    def match_host_resume(self, data, offsets, states, want_results=True, device=0):
        """mfa_match_batch_resume_host: numpy uint8 data, uint64 offsets (n + 1) and uint32 states (n, updated in place) in host memory;
        returns the numpy uint8 results, or None with want_results=False."""
        import numpy as np
        n = len(offsets) - 1
        assert states.dtype == np.uint32 and len(states) >= n
        res = np.zeros(max(n, 1), dtype=np.uint8) if want_results else None
        _check(lib().mfa_match_batch_resume_host(self._h, data.ctypes.data, offsets.ctypes.data, n, states.ctypes.data,
                                                 res.ctypes.data if want_results else None, device), "mfa_match_batch_resume_host")
        return res[:n] if want_results else None

    def match_tensors_resume_set(self, d_bytes, d_offsets, d_states, d_results=None, stream=None):
        """mfa_match_batch_resume_set on torch CUDA tensors: one round of pieces of n strings of a set-walk image, in scan order (a reversed
        image takes a string's LAST piece first).  d_states: int32 or uint32 tensor of n * SET_STATE_WORDS words, updated in place (all zero
        before a string's first piece); d_results: uint8 tensor of n bytes, or None for no result bytes.  Returns d_results.  Asynchronous
        on `stream`."""
        import torch
        n = d_offsets.numel() - 1
        assert d_states.element_size() == 4 and d_states.numel() >= n * SET_STATE_WORDS
        dev = d_offsets.device.index or 0
        s = stream if stream is not None else torch.cuda.current_stream(d_offsets.device)
        _check(lib().mfa_match_batch_resume_set(self._h, d_bytes.data_ptr(), d_offsets.data_ptr(), n, d_states.data_ptr(),
                                                d_results.data_ptr() if d_results is not None else None, dev, ctypes.c_void_p(s.cuda_stream)),
               "mfa_match_batch_resume_set")
        return d_results

    def match_host_resume_set(self, data, offsets, states, want_results=True, device=0):
        """mfa_match_batch_resume_set_host: numpy uint8 data, uint64 offsets (n + 1) and uint32 states (n * SET_STATE_WORDS words, updated in
        place) in host memory; returns the numpy uint8 results, or None with want_results=False."""
        import numpy as np
        n = len(offsets) - 1
        assert states.dtype == np.uint32 and states.size >= n * SET_STATE_WORDS
        res = np.zeros(max(n, 1), dtype=np.uint8) if want_results else None
        _check(lib().mfa_match_batch_resume_set_host(self._h, data.ctypes.data, offsets.ctypes.data, n, states.ctypes.data,
                                                     res.ctypes.data if want_results else None, device), "mfa_match_batch_resume_set_host")
        return res[:n] if want_results else None

    def match_tensors_resume_set_wide(self, d_bytes, d_offsets, d_states, d_results=None, stream=None):
        """mfa_match_batch_resume_set_wide on torch CUDA tensors: one round of pieces of n strings of a wave image (resume_state_bytes() ==
        4 * SET_STATE_WIDE_WORDS), in scan order.  d_states: int32 or uint32 tensor of n * SET_STATE_WIDE_WORDS words, updated in place
        (all zero before a string's first piece); d_results: uint8 tensor of n bytes, or None for no result bytes.  Returns d_results.
        Asynchronous on `stream`."""
        import torch
        n = d_offsets.numel() - 1
        assert d_states.element_size() == 4 and d_states.numel() >= n * SET_STATE_WIDE_WORDS
        dev = d_offsets.device.index or 0
        s = stream if stream is not None else torch.cuda.current_stream(d_offsets.device)
        _check(lib().mfa_match_batch_resume_set_wide(self._h, d_bytes.data_ptr(), d_offsets.data_ptr(), n, d_states.data_ptr(),
                                                     d_results.data_ptr() if d_results is not None else None, dev, ctypes.c_void_p(s.cuda_stream)),
               "mfa_match_batch_resume_set_wide")
        return d_results

    def match_host_resume_set_wide(self, data, offsets, states, want_results=True, device=0):
        """mfa_match_batch_resume_set_wide_host: numpy uint8 data, uint64 offsets (n + 1) and uint32 states (n * SET_STATE_WIDE_WORDS words,
        updated in place) in host memory; returns the numpy uint8 results, or None with want_results=False."""
        import numpy as np
        n = len(offsets) - 1
        assert states.dtype == np.uint32 and states.size >= n * SET_STATE_WIDE_WORDS
        res = np.zeros(max(n, 1), dtype=np.uint8) if want_results else None
        _check(lib().mfa_match_batch_resume_set_wide_host(self._h, data.ctypes.data, offsets.ctypes.data, n, states.ctypes.data,
                                                          res.ctypes.data if want_results else None, device), "mfa_match_batch_resume_set_wide_host")
        return res[:n] if want_results else None

    def resume_state_bytes(self):
        """mfa_image_resume_state_bytes: the bytes of one string's state between two pieces, which names the resume call the image takes --
        0 a memory automaton (none), 4 match_tensors_resume, 48 match_tensors_resume_set, 272 match_tensors_resume_set_wide"""
        out = ctypes.c_uint32()
        _check(lib().mfa_image_resume_state_bytes(self._h, ctypes.byref(out)), "mfa_image_resume_state_bytes")
        return out.value

    def search_tensors(self, d_bytes, d_offsets, d_results=None, d_spans=None, d_span_results=None, stream=None):
        """mfa_search_batch on torch CUDA tensors: the leftmost-longest match inside every string.  d_bytes uint8, d_offsets int64 (n + 1);
        d_results: uint8 tensor of n bytes (None: allocated); d_spans: int64 tensor of 2n + 1 words, or None for results only;
        d_span_results: uint8 tensor of 2n bytes or None (needs d_spans).  Returns d_results[:n].  Asynchronous on `stream`."""
        import torch
        n = d_offsets.numel() - 1
        dev = d_offsets.device.index or 0
        if d_results is None:
            d_results = torch.empty(max(n, 1), dtype=torch.uint8, device=d_offsets.device)
        assert d_spans is None or (d_spans.element_size() == 8 and d_spans.numel() >= 2 * n + 1)
        assert d_span_results is None or (d_span_results.element_size() == 1 and d_span_results.numel() >= 2 * n)
        s = stream if stream is not None else torch.cuda.current_stream(d_offsets.device)
        _check(lib().mfa_search_batch(self._h, d_bytes.data_ptr(), d_offsets.data_ptr(), n, d_results.data_ptr(),
                                      d_spans.data_ptr() if d_spans is not None else None,
                                      d_span_results.data_ptr() if d_span_results is not None else None, dev, ctypes.c_void_p(s.cuda_stream)),
               "mfa_search_batch")
        return d_results[:n]

    def search_host(self, data, offsets, want_spans=True, device=0):
        """mfa_search_batch_host: numpy uint8 data + uint64 offsets (n + 1) in host memory -> (results[n], spans[2n + 1], span_results[2n]),
        the last two None with want_spans=False."""
        import numpy as np
        n = len(offsets) - 1
        res = np.zeros(max(n, 1), dtype=np.uint8)
        spans = np.zeros(2 * n + 1, dtype=np.uint64) if want_spans else None
        sres = np.zeros(max(2 * n, 1), dtype=np.uint8) if want_spans else None
        _check(lib().mfa_search_batch_host(self._h, data.ctypes.data, offsets.ctypes.data, n, res.ctypes.data,
                                           spans.ctypes.data if want_spans else None, sres.ctypes.data if want_spans else None, device),
               "mfa_search_batch_host")
        return res[:n], spans, sres[:2 * n] if want_spans else None

    def search_info(self):
        """mfa_image_search_info: (sets of the pass 1 table, sets of the pass 2 table), the dead set included; raises ERR_UNSUPPORTED for an
        image the search refuses"""
        a, b = ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib().mfa_image_search_info(self._h, ctypes.byref(a), ctypes.byref(b)), "mfa_image_search_info")
        return a.value, b.value

    def last_kernel_ms(self, device=0):
        ms = ctypes.c_float()
        _check(lib().mfa_last_kernel_ms(self._h, device, ctypes.byref(ms)), "mfa_last_kernel_ms")
        return ms.value

    def last_dfa_split(self, device=0):
        """(strings, chunks, chunk_bytes) of the split path for long strings in the last match call; (0, 0, 0) if it did not run"""
        st, ch, cb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
        _check(lib().mfa_last_dfa_split(self._h, device, ctypes.byref(st), ctypes.byref(ch), ctypes.byref(cb)), "mfa_last_dfa_split")
        return st.value, ch.value, cb.value

    def last_dfa_spec(self, device=0):
        """(rewalked_chunks, serial_strings, serial_bytes) of the split path for long strings on a table in L2 in the last match call: what
        repairing the guessed start states cost; (0, 0, 0) if that path did not run"""
        rw, ss, sb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().mfa_last_dfa_spec(self._h, device, ctypes.byref(rw), ctypes.byref(ss), ctypes.byref(sb)), "mfa_last_dfa_spec")
        return rw.value, ss.value, sb.value

    def last_set_split(self, device=0):
        """(strings, chunks, chunk_bytes, rewalked_chunks, serial_strings, serial_bytes) of the split path for long strings of a set-walk
        image in the last match call; all 0 if it did not run"""
        st, ch, cb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
        rw, ss, sb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().mfa_last_set_split(self._h, device, ctypes.byref(st), ctypes.byref(ch), ctypes.byref(cb), ctypes.byref(rw), ctypes.byref(ss),
                                        ctypes.byref(sb)), "mfa_last_set_split")
        return st.value, ch.value, cb.value, rw.value, ss.value, sb.value

    def close(self):
        if self._h:
            lib().mfa_image_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Mixed:
    """A mixed-batch handle (mfa_mixed_t*): several automata, with or without memory, matched against the segments of ONE batch."""

    def __init__(self, images):
        self._images = list(images)                      # the images must outlive the handle
        self._h = ctypes.c_void_p()
        arr = (ctypes.c_void_p * len(self._images))(*[im._h for im in self._images])
        _check(lib().mfa_mixed_create(arr, len(self._images), ctypes.byref(self._h)), "mfa_mixed_create")

    def match_tensors(self, d_bytes, d_offsets, seg_first, d_results=None, stream=None, total_bytes=0):
        """seg_first: host sequence of len(images) + 1 string indices.  Asynchronous on `stream` (default: the current one).
        total_bytes: the batch's size in bytes if the caller knows it (mfa_match_mixed_sized: nothing is read back)."""
        import torch
        n = d_offsets.numel() - 1
        dev = d_offsets.device.index or 0
        if d_results is None:
            d_results = torch.empty(max(n, 1), dtype=torch.uint8, device=d_offsets.device)
        s = stream if stream is not None else torch.cuda.current_stream(d_offsets.device)
        sf = (ctypes.c_uint64 * len(seg_first))(*[int(x) for x in seg_first])
        if total_bytes:
            _check(lib().mfa_match_mixed_sized(self._h, d_bytes.data_ptr(), d_offsets.data_ptr(), n, int(total_bytes), sf, d_results.data_ptr(), dev,
                                               ctypes.c_void_p(s.cuda_stream)), "mfa_match_mixed_sized")
        else:
            _check(lib().mfa_match_mixed(self._h, d_bytes.data_ptr(), d_offsets.data_ptr(), n, sf, d_results.data_ptr(), dev,
                                         ctypes.c_void_p(s.cuda_stream)), "mfa_match_mixed")
        return d_results[:n]

    def last_launches(self, device=0):
        """what the last call launched: {"region_launches", "walk_launches", "groups", "gated"} ("gated" is always False, kept for compatibility)"""
        v = [ctypes.c_uint32() for _ in range(4)]
        _check(lib().mfa_mixed_last_launches(self._h, device, *[ctypes.byref(x) for x in v]), "mfa_mixed_last_launches")
        return {"region_launches": v[0].value, "walk_launches": v[1].value, "groups": v[2].value, "gated": bool(v[3].value)}

    def last_dfa(self, device=0):
        """what the last call did with its memory-less segments: {"multi_launches", "own_launches", "items", "strings"}"""
        v = [ctypes.c_uint32() for _ in range(3)] + [ctypes.c_uint64()]
        _check(lib().mfa_mixed_last_dfa(self._h, device, *[ctypes.byref(x) for x in v]), "mfa_mixed_last_dfa")
        return {"multi_launches": v[0].value, "own_launches": v[1].value, "items": v[2].value, "strings": v[3].value}

    def last_ms(self, device=0, back=0):
        """(region launches, first region launch to last walk) of the call `back` calls ago (0 = the last one), in ms"""
        r, sp = ctypes.c_float(), ctypes.c_float()
        _check(lib().mfa_mixed_timing(self._h, device, back, ctypes.byref(r), ctypes.byref(sp)), "mfa_mixed_timing")
        return r.value, sp.value

    def close(self):
        if self._h:
            lib().mfa_mixed_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def region_scan(d_bytes, d_offsets, d_table=None, stream=None):
    """mfa_region_scan on torch CUDA tensors: returns the region table, int64 [n, REGION_WORDS]."""
    import torch
    n = d_offsets.numel() - 1
    dev = d_offsets.device.index or 0
    if d_table is None:
        d_table = torch.empty((max(n, 1), REGION_WORDS), dtype=torch.int64, device=d_offsets.device)
    s = stream if stream is not None else torch.cuda.current_stream(d_offsets.device)
    _check(lib().mfa_region_scan(d_bytes.data_ptr(), d_offsets.data_ptr(), n, d_table.data_ptr(), dev,
                                 ctypes.c_void_p(s.cuda_stream)), "mfa_region_scan")
    return d_table


def pack_result_bitmap(d_results, d_bitmap=None, stream=None):
    """mfa_pack_result_bitmap on a torch CUDA uint8 result vector: uint8 bitmap ((n + 7) // 8), bit k % 8 of byte k // 8 = string k accepted."""
    import torch
    n = d_results.numel()
    if d_bitmap is None:
        d_bitmap = torch.empty((n + 7) // 8, dtype=torch.uint8, device=d_results.device)
    s = stream if stream is not None else torch.cuda.current_stream(d_results.device)
    _check(lib().mfa_pack_result_bitmap(d_results.data_ptr(), n, d_bitmap.data_ptr(), ctypes.c_void_p(s.cuda_stream)), "mfa_pack_result_bitmap")
    return d_bitmap


def split_tile_bytes():
    """mfa_split_tile_bytes: the bytes of text one workgroup of the splitter takes"""
    return lib().mfa_split_tile_bytes()


def split_workspace_bytes(n_text_bytes):
    out = ctypes.c_size_t()
    _check(lib().mfa_split_workspace_bytes(n_text_bytes, ctypes.byref(out)), "mfa_split_workspace_bytes")
    return out.value


def split_text_count(d_text_ptr, n_text_bytes, mode, stop, d_workspace_ptr, d_info_ptr, device=0, stream=0):
    """mfa_split_text_count on raw device pointers (ints); stop: bytes or None.  Asynchronous on `stream` (a hipStream_t value)."""
    _check(lib().mfa_split_text_count(d_text_ptr, n_text_bytes, mode, stop, d_workspace_ptr, d_info_ptr, device, ctypes.c_void_p(stream)),
           "mfa_split_text_count")


def split_text_write(d_text_ptr, n_text_bytes, mode, d_workspace_ptr, d_info_ptr, d_bytes_ptr, bytes_capacity, d_offsets_ptr, max_strings,
                     device=0, stream=0):
    """mfa_split_text_write on raw device pointers (ints).  Asynchronous on `stream` (a hipStream_t value)."""
    _check(lib().mfa_split_text_write(d_text_ptr, n_text_bytes, mode, d_workspace_ptr, d_info_ptr, d_bytes_ptr, bytes_capacity, d_offsets_ptr,
                                      max_strings, device, ctypes.c_void_p(stream)), "mfa_split_text_write")


def split_text(text, mode, stop=None, stream=None):
    """A text in device memory -> the batch the match calls take.  text: a contiguous torch CUDA uint8 tensor whose memory is 16-byte
    aligned and readable up to its size rounded up to 16 (a tensor with an allocation of its own is; a view into the middle of one
    may not be); mode: SPLIT_LINES or SPLIT_TOKENS; stop: the stop token (bytes, tokens mode only) or None.
    Count, ONE read-back of the 32 bytes of the info record, exact allocation, write -- all on `stream` (default: the current one).
    Returns (bytes, offsets, n, info): a uint8 tensor of n_bytes rounded up to 16 (at least 16) bytes, an int64 tensor of n + 1 offsets,
    the number of strings, and info = {"n_strings", "n_bytes", "stopped"} as read back, plus "d_info": the device record (int64[4]:
    n_strings, n_bytes, max_string_bytes, stopped | overflow << 32), where the write call leaves max_string_bytes."""
    import torch
    assert text.dtype == torch.uint8 and text.is_cuda and text.is_contiguous()
    n_text = text.numel()
    dev = text.device.index or 0
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(text.device)):      # (allocations belong to that stream too)
        s = torch.cuda.current_stream(text.device).cuda_stream
        ptr = text.data_ptr() if n_text else None
        work = torch.empty(max(split_workspace_bytes(n_text), 16), dtype=torch.uint8, device=text.device)
        d_info = torch.zeros(4, dtype=torch.int64, device=text.device)
        split_text_count(ptr, n_text, mode, stop, work.data_ptr(), d_info.data_ptr(), dev, s)
        head = [int(x) for x in d_info.cpu()]                 # the one read-back (it waits for the count)
        n, n_bytes = head[0], head[1]
        d_bytes = torch.empty(max((n_bytes + 15) // 16 * 16, 16), dtype=torch.uint8, device=text.device)
        d_offsets = torch.empty(n + 1, dtype=torch.int64, device=text.device)
        split_text_write(ptr, n_text, mode, work.data_ptr(), d_info.data_ptr(), d_bytes.data_ptr(), d_bytes.numel(), d_offsets.data_ptr(), n, dev, s)
    return d_bytes, d_offsets, n, {"n_strings": n, "n_bytes": n_bytes, "stopped": head[3] & 0xffffffff, "d_info": d_info}


def select_workspace_bytes(n_strings):
    out = ctypes.c_size_t()
    _check(lib().mfa_select_workspace_bytes(n_strings, ctypes.byref(out)), "mfa_select_workspace_bytes")
    return out.value


def select_count(d_results_ptr, d_offsets_ptr, n, flags, d_workspace_ptr, d_info_ptr, device=0, stream=0):
    """mfa_select_count on raw device pointers (ints).  Asynchronous on `stream` (a hipStream_t value)."""
    _check(lib().mfa_select_count(d_results_ptr, d_offsets_ptr, n, flags, d_workspace_ptr, d_info_ptr, device, ctypes.c_void_p(stream)),
           "mfa_select_count")


def select_write(d_bytes_ptr, d_offsets_ptr, d_results_ptr, n, flags, d_workspace_ptr, d_info_ptr, d_out_bytes_ptr, bytes_capacity,
                 d_out_offsets_ptr, d_out_indices_ptr, max_selected, device=0, stream=0):
    """mfa_select_write on raw device pointers (ints; d_out_indices_ptr and, with no capacity, d_out_bytes_ptr may be None).  Asynchronous
    on `stream` (a hipStream_t value)."""
    _check(lib().mfa_select_write(d_bytes_ptr, d_offsets_ptr, d_results_ptr, n, flags, d_workspace_ptr, d_info_ptr, d_out_bytes_ptr,
                                  bytes_capacity, d_out_offsets_ptr, d_out_indices_ptr, max_selected, device, ctypes.c_void_p(stream)),
           "mfa_select_write")


def select(d_bytes, d_offsets, d_results, flags=0, stream=None):
    """The strings of a batch that a match call answered 1 (0 with SELECT_INVERT), compacted on the device.  d_bytes, d_offsets: the batch
    as the match calls take it (torch CUDA uint8 and int64 tensors, n + 1 offsets); d_results: its n result bytes; flags: SELECT_INVERT,
    SELECT_NEWLINE.  Count, ONE read-back of the 32 bytes of the info record, exact allocation, write -- all on `stream` (default: the
    current one).  Returns (out_bytes, out_offsets, out_indices, info): a uint8 tensor of n_bytes rounded up to 16 (at least 16) bytes, of
    which the first n_bytes are the output; int64 tensors of n_selected + 1 offsets and n_selected indices; and info = {"n_selected",
    "n_bytes", "n_unanswered"} as read back, plus "d_info": the device record (int64[4]), where the write call leaves overflow."""
    import torch
    assert d_bytes.dtype == torch.uint8 and d_results.dtype == torch.uint8 and d_offsets.dtype == torch.int64
    assert d_bytes.is_cuda and d_offsets.is_contiguous() and d_results.is_contiguous() and d_bytes.is_contiguous()
    n = d_offsets.numel() - 1
    assert n >= 0 and d_results.numel() >= n
    dev = d_bytes.device.index or 0
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(d_bytes.device)):      # (allocations belong to that stream too)
        s = torch.cuda.current_stream(d_bytes.device).cuda_stream
        work = torch.empty(max(select_workspace_bytes(n), 16), dtype=torch.uint8, device=d_bytes.device)
        d_info = torch.zeros(4, dtype=torch.int64, device=d_bytes.device)
        select_count(d_results.data_ptr(), d_offsets.data_ptr(), n, flags, work.data_ptr(), d_info.data_ptr(), dev, s)
        head = [int(x) for x in d_info.cpu()]                 # the one read-back (it waits for the count)
        n_selected, n_bytes = head[0], head[1]
        out_bytes = torch.empty(max((n_bytes + 15) // 16 * 16, 16), dtype=torch.uint8, device=d_bytes.device)
        out_offsets = torch.empty(n_selected + 1, dtype=torch.int64, device=d_bytes.device)
        out_indices = torch.empty(n_selected, dtype=torch.int64, device=d_bytes.device)
        select_write(d_bytes.data_ptr(), d_offsets.data_ptr(), d_results.data_ptr(), n, flags, work.data_ptr(), d_info.data_ptr(),
                     out_bytes.data_ptr(), out_bytes.numel(), out_offsets.data_ptr(), out_indices.data_ptr() if n_selected else None, n_selected, dev, s)
    return out_bytes, out_offsets, out_indices, {"n_selected": n_selected, "n_bytes": n_bytes, "n_unanswered": head[2], "d_info": d_info}


def device_count():
    return lib().mfa_device_count()
