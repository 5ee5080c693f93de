"""ctypes binding of the C ABI in include/vcfx_gpu.h (libvcfx_gpu.so).

This is plumbing for tests and bench.py; the CLI drop-ins call the same ABI from C++."""
import ctypes
import os

from . import GPU_LIB

VCFXG_OK = 0
MODE_FILE, MODE_STDIN = 0, 1
STATUS = {0: "skip", 1: "row", 2: "drop", 3: "warn", 4: "header"}


class Summary(ctypes.Structure):
    _fields_ = [("n_lines", ctypes.c_uint64), ("rows", ctypes.c_uint64), ("data_lines", ctypes.c_uint64),
                ("warn_lines", ctypes.c_uint64), ("text_bytes", ctypes.c_uint64),
                ("general_records", ctypes.c_uint64)]


class AcParams(ctypes.Structure):
    _fields_ = [("sample", ctypes.c_void_p), ("m", ctypes.c_uint64), ("names", ctypes.c_char_p),
                ("name_off", ctypes.c_void_p), ("seq", ctypes.c_int), ("kind", ctypes.c_int)]


class IbParams(ctypes.Structure):
    _fields_ = [("n_samples", ctypes.c_uint32), ("names", ctypes.c_char_p), ("name_off", ctypes.c_void_p),
                ("freq_mode", ctypes.c_int), ("skip_boundary", ctypes.c_int),
                ("count_boundary_as_used", ctypes.c_int)]


class SxParams(ctypes.Structure):
    _fields_ = [("cols", ctypes.c_void_p), ("m", ctypes.c_uint64), ("mode", ctypes.c_int),
                ("seen_chrom", ctypes.c_int)]


class MsEntry(ctypes.Structure):
    _fields_ = [("id", ctypes.c_char_p), ("id_len", ctypes.c_uint32), ("section", ctypes.c_uint8),
                ("number", ctypes.c_uint8)]


class MsParams(ctypes.Structure):
    _fields_ = [("table", ctypes.c_void_p), ("n_entries", ctypes.c_uint64), ("mode", ctypes.c_int)]


class HxParams(ctypes.Structure):
    """vcfxg_hx_params"""
    _fields_ = [("mode", ctypes.c_int), ("n_samples", ctypes.c_uint32), ("block_size", ctypes.c_int64),
                ("check", ctypes.c_int)]


class FxCol(ctypes.Structure):
    """vcfxg_fx_col"""
    _fields_ = [("kind", ctypes.c_uint32), ("col", ctypes.c_uint32), ("named", ctypes.c_uint32),
                ("key_off", ctypes.c_uint32), ("key_len", ctypes.c_uint32), ("sub_off", ctypes.c_uint32),
                ("sub_len", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class FaParams(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("n_samples", ctypes.c_uint32), ("first_col", ctypes.c_uint64),
                ("total_cols", ctypes.c_uint64), ("row_off", ctypes.c_void_p), ("skip", ctypes.c_void_p)]


class DfParams(ctypes.Structure):
    _fields_ = [("second_start", ctypes.c_uint64), ("assume_sorted", ctypes.c_int), ("natural", ctypes.c_int),
                ("hash_bits", ctypes.c_uint32)]


class MgParams(ctypes.Structure):
    _fields_ = [("file_start", ctypes.c_void_p), ("n_files", ctypes.c_uint32), ("assume_sorted", ctypes.c_int),
                ("natural", ctypes.c_int)]


class CcParams(ctypes.Structure):
    _fields_ = [("n_samples", ctypes.c_uint32), ("mult", ctypes.c_void_p), ("n_mult", ctypes.c_uint64),
                ("threads", ctypes.c_uint64)]


class Criterion(ctypes.Structure):
    _fields_ = [("target", ctypes.c_int), ("op", ctypes.c_int), ("numeric", ctypes.c_int), ("value", ctypes.c_double),
                ("key", ctypes.c_char_p), ("key_len", ctypes.c_size_t), ("str", ctypes.c_char_p),
                ("str_len", ctypes.c_size_t)]


# record_filter criterion codes (vcfx_gpu.h vcfxg_criterion)
POS, QUAL, FILTER, INFO = 0, 1, 2, 3
GT, GE, LT, LE, EQ, NE = 0, 1, 2, 3, 4, 5


# every exported entry point: name -> (restype, argtypes)
_P, _VP, _S, _U64, _I = ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int
SIGNATURES = {
    "vcfxg_version": (_P, []),
    "vcfxg_device_count": (_I, [ctypes.POINTER(_I)]),
    "vcfxg_open": (_I, [_I, ctypes.POINTER(_VP)]),
    "vcfxg_close": (None, [_VP]),
    "vcfxg_device_bytes_live": (_U64, []),
    "vcfxg_last_error": (_P, [_VP]),
    "vcfxg_stream": (_VP, [_VP]),
    "vcfxg_set_profiling": (_I, [_VP, _I]),
    "vcfxg_set_profiling_only": (_I, [_VP, _P]),
    "vcfxg_kernel_ms": (_I, [_VP, _P, ctypes.POINTER(ctypes.c_float)]),
    "vcfxg_kernel_stats": (_I, [_VP, _P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_U64)]),
    "vcfxg_reset_kernel_stats": (_I, [_VP]),
    "vcfxg_load_host": (_I, [_VP, _VP, _S]),
    "vcfxg_ingest_begin": (_I, [_VP, _S]),
    "vcfxg_ingest": (_I, [_VP, _VP, _S, _I]),
    "vcfxg_ingest_wait": (_I, [_VP, _S]),
    "vcfxg_ingest_bgzf": (_I, [_VP, _VP, _S, _VP, _S, _VP, _S, ctypes.POINTER(_U64)]),
    "vcfxg_bgzf_stage": (_I, [_VP, _VP, _S, _S, _S]),
    "vcfxg_bgzf_inflate": (_I, [_VP, _VP, _S]),
    "vcfxg_host_alloc": (_I, [_VP, _S, ctypes.POINTER(_VP)]),
    "vcfxg_host_free": (None, [_VP, _VP]),
    "vcfxg_input_device_ptr": (_VP, [_VP]),
    "vcfxg_input_fetch": (_I, [_VP, _U64, _S, _VP]),
    "vcfxg_index": (_I, [_VP, _S, ctypes.POINTER(_U64)]),
    "vcfxg_line_ends": (_I, [_VP, _U64, _U64, _VP]),
    "vcfxg_allele_freq": (_I, [_VP, _I, ctypes.POINTER(Summary)]),
    "vcfxg_allele_freq_region": (_I, [_VP, _S, _I, ctypes.POINTER(Summary)]),
    "vcfxg_genotype_query": (_I, [_VP, _P, _S, _I, _I, ctypes.POINTER(Summary)]),
    "vcfxg_record_filter": (_I, [_VP, _VP, _I, _I, ctypes.POINTER(Summary)]),
    "vcfxg_record_filter_ex": (_I, [_VP, _VP, _I, _I, _I, ctypes.POINTER(Summary)]),
    "vcfxg_variant_count": (_I, [_VP, _I, ctypes.POINTER(Summary)]),
    "vcfxg_nonref_filter": (_I, [_VP, _I, ctypes.POINTER(Summary)]),
    "vcfxg_nonref_filter_region": (_I, [_VP, _S, _I, ctypes.POINTER(Summary)]),
    "vcfxg_hwe_region": (_I, [_VP, _S, _I, ctypes.POINTER(Summary)]),
    "vcfxg_hwe_rechecks": (_I, [_VP, _VP, _U64, ctypes.POINTER(_U64)]),
    "vcfxg_dosage_region": (_I, [_VP, _S, _I, ctypes.POINTER(Summary)]),
    "vcfxg_missing_region": (_I, [_VP, _S, _I, ctypes.POINTER(Summary)]),
    "vcfxg_allele_counter": (_I, [_VP, _U64, _U64, _VP, ctypes.POINTER(Summary)]),
    "vcfxg_inbreeding_region": (_I, [_VP, _S, _I, _VP, ctypes.POINTER(Summary)]),
    "vcfxg_inbreeding_samples": (_I, [_VP, _VP, _VP, _VP]),
    "vcfxg_sample_extract": (_I, [_VP, _U64, _U64, _VP, ctypes.POINTER(Summary)]),
    "vcfxg_concordance_region": (_I, [_VP, _S, _I, _VP, ctypes.POINTER(Summary)]),
    "vcfxg_concordance_totals": (_I, [_VP, _VP]),
    "vcfxg_chrom_lines": (_I, [_VP, _S, _VP, _U64, ctypes.POINTER(_U64)]),
    "vcfxg_dedup": (_I, [_VP, _I, _VP, ctypes.POINTER(Summary)]),
    "vcfxg_dedup_status": (_I, [_VP, _U64, _U64, _VP]),
    "vcfxg_dedup_counts": (_I, [_VP, _VP]),
    "vcfxg_sort": (_I, [_VP, _I, _VP, ctypes.POINTER(Summary)]),
    "vcfxg_sort_status": (_I, [_VP, _U64, _U64, _VP]),
    "vcfxg_sort_counts": (_I, [_VP, _VP]),
    "vcfxg_sort_order": (_I, [_VP, _U64, _U64, _VP]),
    "vcfxg_sort_text": (_I, [_VP, _U64, ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "vcfxg_diff": (_I, [_VP, _VP, ctypes.POINTER(Summary)]),
    "vcfxg_diff_status": (_I, [_VP, _U64, _U64, _VP]),
    "vcfxg_diff_counts": (_I, [_VP, _VP]),
    "vcfxg_diff_text": (_I, [_VP, _I, _U64, ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "vcfxg_merge": (_I, [_VP, _VP, ctypes.POINTER(Summary)]),
    "vcfxg_merge_status": (_I, [_VP, _U64, _U64, _VP]),
    "vcfxg_merge_counts": (_I, [_VP, _VP]),
    "vcfxg_merge_files": (_I, [_VP, _VP, _VP]),
    "vcfxg_merge_order": (_I, [_VP, _U64, _U64, _VP]),
    "vcfxg_merge_text": (_I, [_VP, _U64, ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "vcfxg_regions_load": (_I, [_VP, _VP, _VP, ctypes.c_uint32, _VP, _VP, _VP, _U64, _VP]),
    "vcfxg_regions_merged": (_I, [_VP, _VP, _VP, _VP, _U64, ctypes.POINTER(_U64)]),
    "vcfxg_region_filter": (_I, [_VP, _I, ctypes.POINTER(Summary)]),
    "vcfxg_region_status": (_I, [_VP, _U64, _U64, _VP]),
    "vcfxg_region_counts": (_I, [_VP, _VP]),
    "vcfxg_multiallelic_split": (_I, [_VP, _U64, _U64, _VP, ctypes.POINTER(Summary)]),
    "vcfxg_ms_line_ranges": (_I, [_VP, _U64, _U64, _VP]),
    "vcfxg_haplotype_scan": (_I, [_VP, _VP, ctypes.POINTER(Summary)]),
    "vcfxg_haplotype_lines": (_I, [_VP, _U64, _U64, _VP, _VP, _VP, _VP, _VP]),
    "vcfxg_haplotype_blocks": (_I, [_VP, ctypes.POINTER(Summary)]),
    "vcfxg_haplotype_table": (_I, [_VP, _U64, _U64, _VP, _VP, _VP, _VP, _VP, _VP]),
    "vcfxg_haplotype_text": (_I, [_VP, ctypes.POINTER(Summary)]),
    "vcfxg_fields_load": (_I, [_VP, _VP, ctypes.c_uint32, _VP, ctypes.c_uint32, _I]),
    "vcfxg_fields_scan": (_I, [_VP, _U64, ctypes.POINTER(Summary)]),
    "vcfxg_fields_lines": (_I, [_VP, _U64, _U64, _VP, _VP, _VP]),
    "vcfxg_fields_cells": (_I, [_VP, _U64, _U64, _VP]),
    "vcfxg_fields_text": (_I, [_VP, ctypes.POINTER(Summary)]),
    "vcfxg_fasta_scan": (_I, [_VP, _U64, _U64, _I, ctypes.c_uint32, ctypes.POINTER(Summary)]),
    "vcfxg_fasta_status": (_I, [_VP, _U64, _U64, _VP, _VP]),
    "vcfxg_fasta_begin": (_I, [_VP, _U64]),
    "vcfxg_fasta": (_I, [_VP, _U64, _U64, _VP, ctypes.POINTER(Summary)]),
    "vcfxg_fetch_text_range": (_I, [_VP, _U64, _S, _VP]),
    "vcfxg_shard_cuts": (_I, [_VP, _S, _S, _I, _VP]),
    "vcfxg_comm_init": (_I, [_VP, _I, ctypes.POINTER(_VP)]),
    "vcfxg_comm_allreduce_u64": (_I, [_VP, _I, _VP, _S]),
    "vcfxg_comm_uses_rccl": (_I, [_VP]),
    "vcfxg_comm_destroy": (None, [_VP]),
    "vcfxg_comm_rccl_stats": (_I, [_VP, ctypes.POINTER(_U64), ctypes.POINTER(_U64)]),
    "vcfxg_last_schedule": (_P, [_VP]),
    "vcfxg_last_af_depth": (_I, [_VP, ctypes.POINTER(_I)]),
    "vcfxg_last_walk_layout": (_I, [_VP, ctypes.POINTER(ctypes.c_int64)]),
    "vcfxg_bgzf_handed_over": (_U64, [_VP]),
    "vcfxg_count_byte": (_I, [_VP, _U64, _I, ctypes.POINTER(_U64)]),
    "vcfxg_haplotype_phaser": (_I, [_VP, _S, _I, ctypes.c_double, ctypes.c_uint32, ctypes.POINTER(Summary)]),
    "vcfxg_phaser_variants": (_I, [_VP, _VP, _VP, _VP]),
    "vcfxg_ld_prepare": (_I, [_VP, _I, _I, _P, _S, _I, _I, _I, _I, ctypes.POINTER(_U64)]),
    "vcfxg_ld_prepare_region": (_I, [_VP, _S, _I, _I, _P, _S, _I, _I, _I, _I, ctypes.POINTER(_U64)]),
    "vcfxg_ld_prefixes": (_I, [_VP, _VP, _S, _VP]),
    "vcfxg_ld_matrix": (_I, [_VP, _I, _I, ctypes.POINTER(_U64)]),
    "vcfxg_ld_stream_chunk": (_I, [_VP, _U64, _U64, _U64, ctypes.c_double, _I, ctypes.POINTER(_U64),
                                   ctypes.POINTER(_U64)]),
    "vcfxg_ld_fetch_pairs": (_I, [_VP, _U64, _U64, _VP, _VP, _VP]),
    "vcfxg_selftest_mfma_i8": (_I, [_VP, ctypes.POINTER(_I)]),
    "vcfxg_selftest_mfma_fp4": (_I, [_VP, ctypes.POINTER(_I)]),
    "vcfxg_filter_query": (_I, [_VP, _VP, _I, _I, _P, _S, _I, ctypes.POINTER(Summary)]),
    "vcfxg_record_filter_region": (_I, [_VP, _S, _VP, _I, _I, ctypes.POINTER(Summary)]),
    "vcfxg_genotype_query_region": (_I, [_VP, _S, _P, _S, _I, _I, ctypes.POINTER(Summary)]),
    "vcfxg_filter_query_region": (_I, [_VP, _S, _VP, _I, _I, _P, _S, _I, ctypes.POINTER(Summary)]),
    "vcfxg_fetch_text": (_I, [_VP, _VP, _S]),
    "vcfxg_fetch_lines": (_I, [_VP, _U64, _U64, _VP, _VP, _VP]),
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(GPU_LIB):
            raise RuntimeError("libvcfx_gpu.so not built (run `make` or __graft_entry__.build())")
        _lib = ctypes.CDLL(GPU_LIB)
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("VCFXG_GPU_LIB") and not hasattr(_lib, name):
                continue  # an older experiment build (A/B runs): its missing entries are not called
            f = getattr(_lib, name)
            f.restype = res
            f.argtypes = args
    return _lib


def device_bytes_live():
    """the device bytes the buffers of this process's open contexts hold (vcfxg_device_bytes_live)"""
    return int(lib().vcfxg_device_bytes_live())


class EngineError(RuntimeError):
    pass


class Engine:
    """One device context (vcfxg_ctx)."""

    def __init__(self, device=0):
        self.L = lib()
        h = ctypes.c_void_p()
        rc = self.L.vcfxg_open(device, ctypes.byref(h))
        if rc != VCFXG_OK:
            raise EngineError("vcfxg_open(%d) failed rc=%d: no usable gfx950 device" % (device, rc))
        self.h = h
        self._buf = None

    def close(self):
        if self.h:
            self.L.vcfxg_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != VCFXG_OK:
            raise EngineError("%s failed rc=%d: %s" % (what, rc, self.L.vcfxg_last_error(self.h).decode()))

    @property
    def stream(self):
        return self.L.vcfxg_stream(self.h)

    def set_profiling(self, on=True):
        self._chk(self.L.vcfxg_set_profiling(self.h, int(on)), "set_profiling")

    def set_profiling_only(self, name=None):
        """time only the named kernel (None: every kernel)"""
        if not hasattr(self.L, "vcfxg_set_profiling_only"):  # (an older experiment build: every kernel)
            return
        self._chk(self.L.vcfxg_set_profiling_only(self.h, name.encode() if name else None), "set_profiling_only")

    def kernel_ms(self, name):
        v = ctypes.c_float()
        rc = self.L.vcfxg_kernel_ms(self.h, name.encode(), ctypes.byref(v))
        return v.value if rc == VCFXG_OK else None

    def kernel_stats(self, name):
        """(total ms, launches) accumulated since reset_kernel_stats()."""
        t = ctypes.c_double()
        n = ctypes.c_uint64()
        self._chk(self.L.vcfxg_kernel_stats(self.h, name.encode(), ctypes.byref(t), ctypes.byref(n)), "kernel_stats")
        return t.value, n.value

    def reset_kernel_stats(self):
        self._chk(self.L.vcfxg_reset_kernel_stats(self.h), "reset_kernel_stats")

    def load(self, data):
        """data: bytes / bytearray / numpy uint8 array (kept alive until the next load)."""
        import numpy as np
        arr = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data
        self._buf = arr
        self._chk(self.L.vcfxg_load_host(self.h, arr.ctypes.data, arr.size), "load_host")

    def ingest(self, chunks):
        """Streaming load: vcfxg_ingest_begin + one vcfxg_ingest per chunk (the last is final)."""
        import numpy as np
        arrs = [np.frombuffer(c, np.uint8) if not isinstance(c, np.ndarray) else c for c in chunks]
        self._buf = arrs
        self._chk(self.L.vcfxg_ingest_begin(self.h, 0), "ingest_begin")
        if not arrs:
            self._chk(self.L.vcfxg_ingest(self.h, None, 0, 1), "ingest")
        for i, a in enumerate(arrs):
            self._chk(self.L.vcfxg_ingest(self.h, a.ctypes.data, a.size, int(i == len(arrs) - 1)), "ingest")

    def load_bgzf(self, comp, members=None, head=b""):
        """vcfxg_ingest_begin + vcfxg_ingest_bgzf + the final vcfxg_ingest: the BGZF members of
        `comp` inflated on the device into the input.  members: bgzf_members(comp) by default.
        Returns None, or (first bad member, error text) when the device refused a member (the
        input is then not loaded)."""
        import numpy as np
        arr = np.frombuffer(comp, np.uint8) if not isinstance(comp, np.ndarray) else comp
        mem = bgzf_members(arr) if members is None else members
        hd = np.frombuffer(head, np.uint8) if head else None
        self._buf = (arr, mem, hd)
        total = int(mem["out_len"].sum()) if len(mem) else 0
        self._chk(self.L.vcfxg_ingest_begin(self.h, total), "ingest_begin")
        bad = ctypes.c_uint64()
        rc = self.L.vcfxg_ingest_bgzf(self.h, arr.ctypes.data, arr.size, mem.ctypes.data if len(mem) else None,
                                      len(mem), hd.ctypes.data if hd is not None else None,
                                      0 if hd is None else hd.size, ctypes.byref(bad))
        if rc == -7:  # VCFXG_E_DATA
            return bad.value, self.L.vcfxg_last_error(self.h).decode()
        self._chk(rc, "ingest_bgzf")
        self._chk(self.L.vcfxg_ingest(self.h, None, 0, 1), "ingest")
        return None

    def bgzf_handed_over(self):
        """members of the last load_bgzf the lane decoder handed to the wave decoder"""
        return int(self.L.vcfxg_bgzf_handed_over(self.h))

    def input_bytes(self, offset, n):
        """bytes [offset, offset + n) of the loaded device input (vcfxg_input_fetch)"""
        b = ctypes.create_string_buffer(max(1, n))
        self._chk(self.L.vcfxg_input_fetch(self.h, offset, n, b), "input_fetch")
        return b.raw[:n]

    def index(self, data_start):
        n = ctypes.c_uint64()
        self._chk(self.L.vcfxg_index(self.h, data_start, ctypes.byref(n)), "index")
        return n.value

    def allele_freq(self, mode=MODE_FILE):
        s = Summary()
        self._chk(self.L.vcfxg_allele_freq(self.h, mode, ctypes.byref(s)), "allele_freq")
        return s

    def allele_freq_region(self, data_start, mode=MODE_FILE):
        """index + allele counts + rows in one fused device sweep (vcfxg_allele_freq_region)."""
        s = Summary()
        self._chk(self.L.vcfxg_allele_freq_region(self.h, data_start, mode, ctypes.byref(s)), "allele_freq_region")
        return s

    def last_af_depth(self):
        """(depth in wave-steps, rolling) of the last AF walk over GT-only records; (0, False): none yet."""
        r = ctypes.c_int()
        d = self.L.vcfxg_last_af_depth(self.h, ctypes.byref(r))
        return d, bool(r.value)

    def last_walk_layout(self):
        """The chunk layout of the last AF walk over GT-only records: a dict with its kind ("uniform", "fit",
        "taper", "split"; None: no such walk yet), C, Cs, K1 (-1: no short round), grid, walkers, resident,
        div and g."""
        out = (ctypes.c_int64 * 8)()
        kind = self.L.vcfxg_last_walk_layout(self.h, out)
        d = dict(zip(("C", "Cs", "K1", "grid", "walkers", "resident", "div", "g"), [int(v) for v in out]))
        d["kind"] = (None, "uniform", "fit", "taper", "split")[kind]
        return d

    def genotype_query(self, query, strict=False, strip_cr=False):
        q = query.encode() if isinstance(query, str) else query
        s = Summary()
        self._chk(self.L.vcfxg_genotype_query(self.h, q, len(q), int(strict), int(strip_cr), ctypes.byref(s)),
                  "genotype_query")
        return s

    def nonref_filter(self, mode):
        """VCFX_nonref_filter per line over the indexed region (mode MODE_FILE / MODE_STDIN)"""
        s = Summary()
        self._chk(self.L.vcfxg_nonref_filter(self.h, int(mode), ctypes.byref(s)), "nonref_filter")
        return s

    def nonref_filter_region(self, data_start, mode):
        """index + nonref_filter in one call (the walk for long records)"""
        s = Summary()
        self._chk(self.L.vcfxg_nonref_filter_region(self.h, data_start, int(mode), ctypes.byref(s)),
                  "nonref_filter_region")
        return s

    def hwe_region(self, data_start, mode):
        """VCFX_hwe_tester over [data_start, n): counts, row rules and rows (vcfxg_hwe_region)"""
        s = Summary()
        self._chk(self.L.vcfxg_hwe_region(self.h, data_start, int(mode), ctypes.byref(s)), "hwe_region")
        return s

    def dosage_region(self, data_start, mode):
        """VCFX_dosage_calculator rows over the data lines from data_start (vcfxg_dosage_region)"""
        s = Summary()
        self._chk(self.L.vcfxg_dosage_region(self.h, data_start, int(mode), ctypes.byref(s)), "dosage_region")
        return s

    def missing_region(self, data_start, mode):
        """VCFX_missing_detector's per-line test over the lines from data_start (vcfxg_missing_region)"""
        s = Summary()
        self._chk(self.L.vcfxg_missing_region(self.h, data_start, int(mode), ctypes.byref(s)), "missing_region")
        return s

    def allele_counter(self, l0, l1, samples, names, seq=0, kind=0):
        """VCFX_allele_counter rows of indexed lines [l0, l1) for the output slots (sample index,
        name) (vcfxg_allele_counter); seq 0 = the file path's every-slot semantics, 1 = the
        forward cursor; kind 0 text, 1 aggregate, 2 binary"""
        import numpy as np
        idx = np.ascontiguousarray(samples, np.uint32)
        nb = [x.encode() if isinstance(x, str) else bytes(x) for x in names]
        assert len(nb) == len(idx)
        off = np.zeros(len(nb) + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in nb])
        p = AcParams(idx.ctypes.data, len(idx), b"".join(nb), off.ctypes.data, int(seq), int(kind))
        s = Summary()
        self._chk(self.L.vcfxg_allele_counter(self.h, l0, l1, ctypes.byref(p), ctypes.byref(s)), "allele_counter")
        return s

    def inbreeding_region(self, data_start, mode, names, freq_mode=0, skip_boundary=False,
                          count_boundary_as_used=False):
        """VCFX_inbreeding_calculator over the records from data_start: a row per sample (names:
        the header's sample names; freq_mode 0 excludeSample / 1 global) (vcfxg_inbreeding_region)"""
        import numpy as np
        nb = [x.encode() if isinstance(x, str) else bytes(x) for x in names]
        off = np.zeros(len(nb) + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in nb])
        p = IbParams(len(nb), b"".join(nb), off.ctypes.data, int(freq_mode), int(skip_boundary),
                     int(count_boundary_as_used))
        s = Summary()
        self._ib_n = 0
        self._chk(self.L.vcfxg_inbreeding_region(self.h, data_start, int(mode), ctypes.byref(p), ctypes.byref(s)),
                  "inbreeding_region")
        self._ib_n = len(nb)
        return s

    def inbreeding_samples(self):
        """(sum_exp float64, obs_het uint64, used uint64) per sample of the last inbreeding_region"""
        import numpy as np
        n = getattr(self, "_ib_n", 0)
        if not n:
            raise EngineError("inbreeding_samples: no successful inbreeding_region call on this context")
        se, oh, us = np.zeros(n, np.float64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        self._chk(self.L.vcfxg_inbreeding_samples(self.h, se.ctypes.data, oh.ctypes.data, us.ctypes.data),
                  "inbreeding_samples")
        return se, oh, us

    def sample_extract(self, l0, l1, cols, mode=MODE_FILE, seen_chrom=True):
        """VCFX_sample_extractor's rewrite of indexed lines [l0, l1) keeping the columns `cols`
        (field numbers >= 9, ascending) (vcfxg_sample_extract).  One call takes at most
        VCFXG_SX_BLOCK lines: the summary's n_lines says how many, and the caller goes on from
        l0 + n_lines; text(s.text_bytes) holds their bytes, statuses their per-line status."""
        import numpy as np
        idx = np.ascontiguousarray(cols, np.uint32)
        p = SxParams(idx.ctypes.data if len(idx) else None, len(idx), int(mode), int(bool(seen_chrom)))
        s = Summary()
        self._chk(self.L.vcfxg_sample_extract(self.h, l0, l1, ctypes.byref(p), ctypes.byref(s)), "sample_extract")
        return s

    def sample_extract_all(self, l0, l1, cols, mode=MODE_FILE, seen_chrom=True):
        """sample_extract block by block over [l0, l1): (text, statuses, summaries)"""
        import numpy as np
        text, st, sums = [], [], []
        while l0 < l1:
            s = self.sample_extract(l0, l1, cols, mode, seen_chrom)
            text.append(self.text(s.text_bytes))
            b = np.zeros(max(int(s.n_lines), 1), np.uint8)
            self._chk(self.L.vcfxg_fetch_lines(self.h, l0, s.n_lines, None, None, b.ctypes.data), "fetch_lines")
            st.append(b[:s.n_lines])
            sums.append(s)
            l0 += s.n_lines
        return b"".join(text), (np.concatenate(st) if st else np.zeros(0, np.uint8)), sums

    def concordance(self, data_start, mode, n_samples=0, mult=None, threads=0):
        """VCFX_cross_sample_concordance over the lines from data_start (vcfxg_concordance_region):
        mult = per sample column how often it is selected (None: each of the first n_samples
        once), threads = T of the file mode's row order (0: record order).  Returns (summary,
        totals, text): totals = (concordant, discordant, no-genotype rows, data lines); per line
        N, U and status through lines(summary.n_lines)."""
        import numpy as np
        m = None if mult is None else np.ascontiguousarray(mult, np.uint32)
        if m is not None and not len(m):
            m = np.zeros(1, np.uint32)  # an empty selection: no column (NULL would select them all)
        p = CcParams(int(n_samples), None if m is None else m.ctypes.data, 0 if m is None else len(m), int(threads))
        s = Summary()
        self._chk(self.L.vcfxg_concordance_region(self.h, data_start, int(mode), ctypes.byref(p), ctypes.byref(s)),
                  "concordance_region")
        t = np.zeros(4, np.uint64)
        self._chk(self.L.vcfxg_concordance_totals(self.h, t.ctypes.data), "concordance_totals")
        return s, tuple(int(x) for x in t), self.text(s.text_bytes)

    def dedup(self, mode, hash_bits=0):
        """VCFX_duplicate_remover's decision over the indexed lines (index(0) first; vcfxg_dedup):
        hash_bits 1..63 keeps only that many low bits of the key hash (forces collisions).  Returns
        (summary, statuses uint8 per line: VCFXG_DD_*, counts per status + the wave-path lines)."""
        import numpy as np
        p = ctypes.c_uint32(int(hash_bits))  # vcfxg_dd_params
        s = Summary()
        self._chk(self.L.vcfxg_dedup(self.h, int(mode), ctypes.byref(p), ctypes.byref(s)), "dedup")
        st = np.zeros(max(int(s.n_lines), 1), np.uint8)
        self._chk(self.L.vcfxg_dedup_status(self.h, 0, s.n_lines, st.ctypes.data), "dedup_status")
        cnt = np.zeros(6, np.uint64)
        self._chk(self.L.vcfxg_dedup_counts(self.h, cnt.ctypes.data), "dedup_counts")
        return s, st[:s.n_lines], tuple(int(x) for x in cnt)

    def regions_load(self, names, chrom_id, start1, end, hash_bits=0):
        """VCFX_region_subsampler's table (vcfxg_regions_load): names = the distinct chromosome names
        (bytes), and per interval its name's index, 1-based start and end.  hash_bits 1..63 keeps
        only that many low bits of the names' hash (forces collisions in the dictionary).  The table
        stays resident until the next call."""
        import numpy as np
        blob = b"".join(names)
        off = np.zeros(len(names) + 1, np.uint64)
        if names:
            off[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
        cid = np.ascontiguousarray(chrom_id, np.uint32)
        s1 = np.ascontiguousarray(start1, np.int32)
        e = np.ascontiguousarray(end, np.int32)
        assert len(cid) == len(s1) == len(e)
        p = ctypes.c_uint32(int(hash_bits))  # vcfxg_rs_params
        self._chk(self.L.vcfxg_regions_load(self.h, blob, off.ctypes.data, len(names), cid.ctypes.data, s1.ctypes.data,
                                            e.ctypes.data, len(cid), ctypes.byref(p)), "regions_load")

    def regions_merged(self):
        """the resident table's merged intervals in (name index, start) order (vcfxg_regions_merged):
        a list of (name index, start, end)"""
        import numpy as np
        n = _U64(0)
        self._chk(self.L.vcfxg_regions_merged(self.h, None, None, None, 0, ctypes.byref(n)), "regions_merged")
        k = int(n.value)
        cid, s1, e = np.zeros(max(k, 1), np.uint32), np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.int32)
        self._chk(self.L.vcfxg_regions_merged(self.h, cid.ctypes.data, s1.ctypes.data, e.ctypes.data, k, ctypes.byref(n)),
                  "regions_merged")
        return list(zip(cid[:k].tolist(), s1[:k].tolist(), e[:k].tolist()))

    def region_filter(self, mode):
        """VCFX_region_subsampler's decision over the indexed lines against the resident table
        (index(0) and regions_load first; vcfxg_region_filter).  Returns (summary, statuses uint8
        per line: VCFXG_RS_*, counts per status + the wave-path lines)."""
        import numpy as np
        s = Summary()
        self._chk(self.L.vcfxg_region_filter(self.h, int(mode), ctypes.byref(s)), "region_filter")
        st = np.zeros(max(int(s.n_lines), 1), np.uint8)
        self._chk(self.L.vcfxg_region_status(self.h, 0, s.n_lines, st.ctypes.data), "region_status")
        cnt = np.zeros(8, np.uint64)
        self._chk(self.L.vcfxg_region_counts(self.h, cnt.ctypes.data), "region_counts")
        return s, st[:s.n_lines], tuple(int(x) for x in cnt)

    def sort(self, mode, natural=False):
        """VCFX_sorter's statuses and order over the indexed lines (index(0) first; vcfxg_sort).
        Returns (summary, statuses uint8 per line: VCFXG_SRT_*, counts per status + the wave-path
        lines, order: the input line number of every output line)."""
        import numpy as np
        p = ctypes.c_int(int(bool(natural)))  # vcfxg_srt_params
        s = Summary()
        self._chk(self.L.vcfxg_sort(self.h, int(mode), ctypes.byref(p), ctypes.byref(s)), "sort")
        st = np.zeros(max(int(s.n_lines), 1), np.uint8)
        self._chk(self.L.vcfxg_sort_status(self.h, 0, s.n_lines, st.ctypes.data), "sort_status")
        cnt = np.zeros(6, np.uint64)
        self._chk(self.L.vcfxg_sort_counts(self.h, cnt.ctypes.data), "sort_counts")
        order = np.zeros(max(int(s.rows), 1), np.uint32)
        self._chk(self.L.vcfxg_sort_order(self.h, 0, s.rows, order.ctypes.data), "sort_order")
        return s, st[:s.n_lines], tuple(int(x) for x in cnt), order[:s.rows]

    def sort_text(self, first):
        """output lines [first, first + lines) of the last sort() gathered on the device, one block
        of at most VCFXG_SRT_BLOCK bytes (vcfxg_sort_text): (lines taken, their bytes)"""
        k, n = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self.L.vcfxg_sort_text(self.h, int(first), ctypes.byref(k), ctypes.byref(n)), "sort_text")
        return k.value, self.text_range(0, n.value)

    def sorted_text(self, rows):
        """the whole output of the last sort() (rows = its summary's rows), block after block"""
        out, j = [], 0
        while j < rows:
            k, text = self.sort_text(j)
            out.append(text)
            j += k
        return b"".join(out)

    def diff(self, second_start, assume_sorted=False, natural=False, hash_bits=0):
        """VCFX_diff_tool over the indexed lines of two files loaded as one text (file 1, a newline if
        it lacks its last one, file 2; index(0) first; vcfxg_diff): second_start = the byte where
        file 2 begins.  Returns (summary, statuses uint8 per line: VCFXG_DF_*, counts: unique lines
        of file 1 and 2, data lines of file 1 and 2, skipped lines, wave-path lines, the path taken,
        the cut line)."""
        import numpy as np
        p = DfParams(int(second_start), int(bool(assume_sorted)), int(bool(natural)), int(hash_bits))
        s = Summary()
        self._chk(self.L.vcfxg_diff(self.h, ctypes.byref(p), ctypes.byref(s)), "diff")
        st = np.zeros(max(int(s.n_lines), 1), np.uint8)
        self._chk(self.L.vcfxg_diff_status(self.h, 0, s.n_lines, st.ctypes.data), "diff_status")
        cnt = np.zeros(8, np.uint64)
        self._chk(self.L.vcfxg_diff_counts(self.h, cnt.ctypes.data), "diff_counts")
        return s, st[:s.n_lines], tuple(int(x) for x in cnt)

    def diff_text(self, side, first):
        """keys [first, first + taken) of one side (0: file 1) of the last diff(), each with its
        newline, one block of at most VCFXG_DF_BLOCK bytes (vcfxg_diff_text): (keys taken, bytes)"""
        k, n = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self.L.vcfxg_diff_text(self.h, int(side), int(first), ctypes.byref(k), ctypes.byref(n)), "diff_text")
        return k.value, self.text_range(0, n.value)

    def diffed_text(self, side):
        """one side's whole output of the last diff(), block after block"""
        cnt = (ctypes.c_uint64 * 8)()
        self._chk(self.L.vcfxg_diff_counts(self.h, ctypes.cast(cnt, ctypes.c_void_p)), "diff_counts")
        out, j = [], 0
        while j < cnt[int(side)]:
            k, text = self.diff_text(side, j)
            out.append(text)
            j += k
        return b"".join(out)

    def merge(self, file_starts, assume_sorted=False, natural=False):
        """VCFX_merger over the indexed lines of K files loaded as one text (every file in list order,
        a newline after one that lacks its last; index(0) first; vcfxg_merge): file_starts = the K + 1
        bytes where the files begin, the last one the text's size.  Returns (summary, statuses uint8
        per line: VCFXG_MG_*, counts: the lines per status, wave-path lines, the path taken, the
        header's file, order: the input line number of every output line)."""
        import numpy as np
        fs = np.ascontiguousarray(file_starts, np.uint64)
        p = MgParams(fs.ctypes.data, len(fs) - 1, int(bool(assume_sorted)), int(bool(natural)))
        s = Summary()
        self._chk(self.L.vcfxg_merge(self.h, ctypes.byref(p), ctypes.byref(s)), "merge")
        st = np.zeros(max(int(s.n_lines), 1), np.uint8)
        self._chk(self.L.vcfxg_merge_status(self.h, 0, s.n_lines, st.ctypes.data), "merge_status")
        cnt = np.zeros(8, np.uint64)
        self._chk(self.L.vcfxg_merge_counts(self.h, cnt.ctypes.data), "merge_counts")
        order = np.zeros(max(int(s.rows), 1), np.uint32)
        self._chk(self.L.vcfxg_merge_order(self.h, 0, s.rows, order.ctypes.data), "merge_order")
        return s, st[:s.n_lines], tuple(int(x) for x in cnt), order[:s.rows]

    def merge_files(self, n_files):
        """each file's first line (n_files + 1 entries) and its BAD lines of the last merge()"""
        import numpy as np
        first, bad = np.zeros(n_files + 1, np.uint64), np.zeros(max(n_files, 1), np.uint64)
        self._chk(self.L.vcfxg_merge_files(self.h, first.ctypes.data, bad.ctypes.data), "merge_files")
        return [int(x) for x in first], [int(x) for x in bad[:n_files]]

    def merge_text(self, first):
        """output lines [first, first + lines) of the last merge() gathered on the device, one block
        of at most VCFXG_SRT_BLOCK bytes (vcfxg_merge_text): (lines taken, their bytes)"""
        k, n = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self.L.vcfxg_merge_text(self.h, int(first), ctypes.byref(k), ctypes.byref(n)), "merge_text")
        return k.value, self.text_range(0, n.value)

    def merged_text(self, rows):
        """the whole output of the last merge() (rows = its summary's rows), block after block"""
        out, j = [], 0
        while j < rows:
            k, text = self.merge_text(j)
            out.append(text)
            j += k
        return b"".join(out)

    def multiallelic_split(self, l0, l1, table, mode=MODE_FILE):
        """VCFX_multiallelic_splitter over indexed lines [l0, l1) (vcfxg_multiallelic_split).  table:
        (id bytes, section 0 INFO / 1 FORMAT, number 0 other / 1 A / 2 R / 3 G) in header order.  One
        call takes a bounded block: returns (summary, statuses, nAlts, offsets, text) of the
        summary's n_lines lines; text holds the rows of the split lines, line i's at
        text[offsets[i]:offsets[i + 1]]; the caller goes on from l0 + n_lines."""
        import numpy as np
        ids = [bytes(t[0]) for t in table]
        ent = (MsEntry * max(len(ids), 1))()
        for e, i, t in zip(ent, ids, table):
            e.id, e.id_len, e.section, e.number = i, len(i), int(t[1]), int(t[2])
        p = MsParams(ctypes.cast(ent, ctypes.c_void_p) if ids else None, len(ids), int(mode))
        s = Summary()
        self._chk(self.L.vcfxg_multiallelic_split(self.h, l0, l1, ctypes.byref(p), ctypes.byref(s)),
                  "multiallelic_split")
        n = int(s.n_lines)
        st, alt, off = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int32), np.zeros(n + 1, np.uint64)
        self._chk(self.L.vcfxg_fetch_lines(self.h, l0, n, alt.ctypes.data, None, st.ctypes.data), "fetch_lines")
        if n:
            self._chk(self.L.vcfxg_ms_line_ranges(self.h, l0, n, off.ctypes.data), "ms_line_ranges")
        return s, st[:n], alt[:n], off, self.text(s.text_bytes)

    def haplotype_scan(self, n_samples, block_size=100000, check=False, mode=MODE_FILE):
        """VCFX_haplotype_extractor's decisions over the indexed lines (index(first data line) first;
        vcfxg_haplotype_scan).  Returns (summary: rows = members, data_lines = blocks; per line status
        uint8 VCFXG_HX_*, pos int64, member, block (uint64, ~0 off the members), flip (uint32: the first
        flipping sample, n_samples for none, ~0 off the members))."""
        import numpy as np
        p = HxParams(int(mode), int(n_samples), int(block_size), int(bool(check)))
        s = Summary()
        self._chk(self.L.vcfxg_haplotype_scan(self.h, ctypes.byref(p), ctypes.byref(s)), "haplotype_scan")
        n = int(s.n_lines)
        st, pos = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int64)
        mem, blk, flip = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint32)
        self._chk(self.L.vcfxg_haplotype_lines(self.h, 0, n, st.ctypes.data, pos.ctypes.data, mem.ctypes.data,
                                               blk.ctypes.data, flip.ctypes.data), "haplotype_lines")
        return s, st[:n], pos[:n], mem[:n], blk[:n], flip[:n]

    def haplotype_blocks(self):
        """the block table of the last haplotype_scan (vcfxg_haplotype_blocks): (summary: rows = blocks,
        text_bytes; per block first member, last member, start, end, row offset, row length)"""
        import numpy as np
        s = Summary()
        self._chk(self.L.vcfxg_haplotype_blocks(self.h, ctypes.byref(s)), "haplotype_blocks")
        nb = int(s.rows)
        a = [np.zeros(max(nb, 1), t) for t in (np.uint64, np.uint64, np.int64, np.int64, np.uint64, np.uint64)]
        self._chk(self.L.vcfxg_haplotype_table(self.h, 0, nb, *[x.ctypes.data for x in a]), "haplotype_table")
        return (s,) + tuple(x[:nb] for x in a)

    def haplotype_text(self):
        """the rows of the last haplotype_blocks written on the device (vcfxg_haplotype_text): their bytes"""
        s = Summary()
        self._chk(self.L.vcfxg_haplotype_text(self.h, ctypes.byref(s)), "haplotype_text")
        return self.text_range(0, int(s.text_bytes)) if s.text_bytes else b""

    def fields_load(self, cols, pool, mode=MODE_FILE):
        """VCFX_field_extractor's table (vcfxg_fields_load): cols = (kind, col, named, key_off, key_len,
        sub_off, sub_len) per output column (kinds and VCFXG_FX_NOKEY as in vcfx_gpu.h), pool = the keys'
        and sub-fields' bytes.  The table stays on the context."""
        arr = (FxCol * max(len(cols), 1))()
        for i, c in enumerate(cols):
            arr[i] = FxCol(*[int(x) for x in c], 0)
        self._fx_ncols = len(cols)
        self._chk(self.L.vcfxg_fields_load(self.h, ctypes.cast(arr, ctypes.c_void_p), len(cols), bytes(pool), len(pool),
                                           int(mode)), "fields_load")

    def fields_scan(self, names_from=0xFFFFFFFFFFFFFFFF):
        """the cell pass over the indexed lines against the resident table (index(0) first;
        vcfxg_fields_scan): (summary: rows, text_bytes, general_records = the table was read from global
        memory; per line status uint8 VCFXG_FX_*, the rows before it, the text bytes before it (uint64);
        the matrix of the ROW lines, rows x columns x (offset, length) uint32).  A named cell holds for the
        lines that start at or after byte names_from."""
        import numpy as np
        s = Summary()
        self._chk(self.L.vcfxg_fields_scan(self.h, int(names_from), ctypes.byref(s)), "fields_scan")
        n, nc = int(s.n_lines), self._fx_ncols
        st, row, off = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
        cells = np.zeros((max(n, 1), nc, 2), np.uint32)
        self._chk(self.L.vcfxg_fields_lines(self.h, 0, n, st.ctypes.data, row.ctypes.data, off.ctypes.data), "fields_lines")
        self._chk(self.L.vcfxg_fields_cells(self.h, 0, n, cells.ctypes.data), "fields_cells")
        st = st[:n]
        return s, st, row[:n], off[:n], cells[:n][st == 2]

    def fields_text(self):
        """the rows of the last fields_scan written on the device (vcfxg_fields_text): their bytes"""
        s = Summary()
        self._chk(self.L.vcfxg_fields_text(self.h, ctypes.byref(s)), "fields_text")
        return self.text_range(0, int(s.text_bytes)) if s.text_bytes else b""

    def fasta_scan(self, l0, l1, n_samples, mode=MODE_FILE):
        """VCFX_fasta_converter's statuses over indexed lines [l0, l1) (vcfxg_fasta_scan; stdin mode
        counts a line's fields against n_samples).  One call takes a bounded block: returns (summary,
        statuses, column numbers within the block) of the summary's n_lines lines."""
        import numpy as np
        s = Summary()
        self._chk(self.L.vcfxg_fasta_scan(self.h, l0, l1, int(mode), int(n_samples), ctypes.byref(s)), "fasta_scan")
        n = int(s.n_lines)
        st, col = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint64)
        if n:
            self._chk(self.L.vcfxg_fasta_status(self.h, l0, n, st.ctypes.data, col.ctypes.data), "fasta_status")
        return s, st[:n], col[:n]

    def fasta_begin(self, text_bytes):
        self._chk(self.L.vcfxg_fasta_begin(self.h, int(text_bytes)), "fasta_begin")

    def fasta(self, l0, l1, n_samples, first_col, total_cols, row_off, skip=None, mode=MODE_FILE):
        """the bases of the columns among indexed lines [l0, l1), transposed into the text sized by
        fasta_begin (vcfxg_fasta): sample s, column first_col + c at row_off[s] + c' + c' // 60 with
        c' = first_col + c - skip[s].  Returns the summary (n_lines taken, rows = columns written,
        general_records); the text is read with text_range."""
        import numpy as np
        ro = np.ascontiguousarray(row_off, np.uint64)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint64)
        p = FaParams(int(mode), int(n_samples), int(first_col), int(total_cols), ro.ctypes.data,
                     None if sk is None else sk.ctypes.data)
        s = Summary()
        self._chk(self.L.vcfxg_fasta(self.h, l0, l1, ctypes.byref(p), ctypes.byref(s)), "fasta")
        return s

    def chrom_lines(self, data_start):
        """start offsets of the lines from data_start that begin with '#CHROM' (vcfxg_chrom_lines)"""
        import numpy as np
        n = ctypes.c_uint64(0)
        out = np.zeros(16, np.uint64)
        self._chk(self.L.vcfxg_chrom_lines(self.h, data_start, out.ctypes.data, len(out), ctypes.byref(n)), "chrom_lines")
        if n.value > len(out):
            out = np.zeros(n.value, np.uint64)
            self._chk(self.L.vcfxg_chrom_lines(self.h, data_start, out.ctypes.data, len(out), ctypes.byref(n)),
                      "chrom_lines")
        return out[:n.value]

    def haplotype_phaser(self, data_start, mode, threshold, n_samples):
        """VCFX_haplotype_phaser's parse + consecutive-variant LD (vcfxg_haplotype_phaser)"""
        s = Summary()
        self._chk(self.L.vcfxg_haplotype_phaser(self.h, data_start, int(mode), float(threshold), int(n_samples),
                                                ctypes.byref(s)), "haplotype_phaser")
        return s

    def phaser_variants(self, n_var):
        """(flags, r2, entry offsets) of the last haplotype_phaser call"""
        import numpy as np
        f = np.zeros(max(n_var, 1), np.uint8)
        r2 = np.zeros(max(n_var, 1), np.float64)
        off = np.zeros(n_var + 1, np.uint64)
        self._chk(self.L.vcfxg_phaser_variants(self.h, f.ctypes.data, r2.ctypes.data, off.ctypes.data),
                  "phaser_variants")
        return f[:n_var], r2[:n_var], off

    def text_range(self, offset, n):
        b = ctypes.create_string_buffer(max(1, n))
        self._chk(self.L.vcfxg_fetch_text_range(self.h, offset, n, b), "fetch_text_range")
        return b.raw[:n]

    def hwe_rechecks(self):
        """the last hwe_region's rows left to the host: [(text_offset, hom_ref, het, hom_alt)]"""
        import numpy as np
        n = ctypes.c_uint64()
        self._chk(self.L.vcfxg_hwe_rechecks(self.h, None, 0, ctypes.byref(n)), "hwe_rechecks")
        a = np.zeros((max(n.value, 1), 3), np.uint64)  # 24 B per vcfxg_hwe_recheck
        self._chk(self.L.vcfxg_hwe_rechecks(self.h, a.ctypes.data, n.value, ctypes.byref(n)), "hwe_rechecks")
        v = a[:n.value].view(np.uint32).reshape(-1, 6)
        return [(int(r[0]) | (int(r[1]) << 32), int(r[2]), int(r[3]), int(r[4])) for r in v]

    def _criteria(self, crits):
        """crits: list of (target, op, numeric, value, key, str) as vcfxg_criterion."""
        arr = (Criterion * max(1, len(crits)))()
        self._keep = []
        for i, (target, op, numeric, value, key, sval) in enumerate(crits):
            k = key.encode() if isinstance(key, str) else key
            s = sval.encode() if isinstance(sval, str) else sval
            self._keep += [k, s]
            arr[i] = Criterion(target, op, int(numeric), float(value), k, len(k), s, len(s))
        return arr

    def record_filter(self, crits, and_logic=True):
        s = Summary()
        arr = self._criteria(crits)
        self._chk(self.L.vcfxg_record_filter(self.h, ctypes.cast(arr, ctypes.c_void_p), len(crits), int(and_logic),
                                             ctypes.byref(s)), "record_filter")
        return s

    def filter_query(self, crits, query, and_logic=True, strict=False):
        s = Summary()
        arr = self._criteria(crits)
        q = query.encode() if isinstance(query, str) else query
        self._chk(self.L.vcfxg_filter_query(self.h, ctypes.cast(arr, ctypes.c_void_p), len(crits), int(and_logic), q,
                                            len(q), int(strict), ctypes.byref(s)), "filter_query")
        return s

    def record_filter_region(self, data_start, crits, and_logic=True):
        """index + record_filter in one call (vcfxg_record_filter_region)."""
        s = Summary()
        arr = self._criteria(crits)
        self._chk(self.L.vcfxg_record_filter_region(self.h, data_start, ctypes.cast(arr, ctypes.c_void_p), len(crits),
                                                    int(and_logic), ctypes.byref(s)), "record_filter_region")
        return s

    def genotype_query_region(self, data_start, query, strict=False, strip_cr=False):
        """index + genotype_query in one call (vcfxg_genotype_query_region)."""
        q = query.encode() if isinstance(query, str) else query
        s = Summary()
        self._chk(self.L.vcfxg_genotype_query_region(self.h, data_start, q, len(q), int(strict), int(strip_cr),
                                                     ctypes.byref(s)), "genotype_query_region")
        return s

    def filter_query_region(self, data_start, crits, query, and_logic=True, strict=False):
        """index + the fused record_filter | genotype_query in one call (vcfxg_filter_query_region)."""
        s = Summary()
        arr = self._criteria(crits)
        q = query.encode() if isinstance(query, str) else query
        self._chk(self.L.vcfxg_filter_query_region(self.h, data_start, ctypes.cast(arr, ctypes.c_void_p), len(crits),
                                                   int(and_logic), q, len(q), int(strict), ctypes.byref(s)),
                  "filter_query_region")
        return s

    def ld_prepare(self, n_samples, id_dot_to_pos=True, region=None):
        n = ctypes.c_uint64()
        rc, rs, re_ = (region[0].encode(), region[1], region[2]) if region else (b"", 0, 0)
        self._chk(self.L.vcfxg_ld_prepare(self.h, n_samples, int(id_dot_to_pos), rc, len(rc), int(bool(region)), rs,
                                          re_, 0, ctypes.byref(n)), "ld_prepare")
        return n.value

    def ld_prepare_region(self, data_start, n_samples, id_dot_to_pos=True, region=None):
        """vcfxg_index + vcfxg_ld_prepare in one call (the LD walk for long records)."""
        n = ctypes.c_uint64()
        rc, rs, re_ = (region[0].encode(), region[1], region[2]) if region else (b"", 0, 0)
        self._chk(self.L.vcfxg_ld_prepare_region(self.h, data_start, n_samples, int(id_dot_to_pos), rc, len(rc),
                                                 int(bool(region)), rs, re_, 0, ctypes.byref(n)), "ld_prepare_region")
        return n.value

    def ld_stream_chunk(self, j0, j1, window, threshold, max_dist=0):
        npairs = ctypes.c_uint64()
        tb = ctypes.c_uint64()
        self._chk(self.L.vcfxg_ld_stream_chunk(self.h, j0, j1, window, threshold, max_dist, ctypes.byref(npairs),
                                               ctypes.byref(tb)), "ld_stream_chunk")
        return npairs.value, tb.value

    def count_byte(self, from_, byte):
        n = ctypes.c_uint64()
        self._chk(self.L.vcfxg_count_byte(self.h, from_, byte, ctypes.byref(n)), "count_byte")
        return n.value

    def ld_prefixes(self, m):
        """The m variants' "CHROM\tPOS\tID" prefixes of the last LD prepare, as a list of bytes."""
        import numpy as np
        offs = np.zeros(m + 1, np.uint64)
        self._chk(self.L.vcfxg_ld_prefixes(self.h, None, 0, offs.ctypes.data) if m == 0 else
                  self.L.vcfxg_ld_prefixes(self.h, None, 1 << 62, offs.ctypes.data), "ld_prefixes")
        text = ctypes.create_string_buffer(int(offs[m]) + 1)
        self._chk(self.L.vcfxg_ld_prefixes(self.h, text, int(offs[m]) + 1, None), "ld_prefixes")
        raw = text.raw
        return [raw[int(offs[k]):int(offs[k + 1])] for k in range(m)]

    def ld_pairs(self, first, count):
        """(i, j, r2) numpy arrays of pairs [first, first + count) of the last ld_stream_chunk."""
        import numpy as np
        vi = np.zeros(count, np.uint32)
        vj = np.zeros(count, np.uint32)
        r2 = np.zeros(count, np.float64)
        self._chk(self.L.vcfxg_ld_fetch_pairs(self.h, first, count, vi.ctypes.data, vj.ctypes.data, r2.ctypes.data),
                  "ld_fetch_pairs")
        return vi, vj, r2

    def selftest_mfma_i8(self):
        m = ctypes.c_int()
        self._chk(self.L.vcfxg_selftest_mfma_i8(self.h, ctypes.byref(m)), "selftest")
        return m.value

    def selftest_mfma_fp4(self):
        m = ctypes.c_int()
        self._chk(self.L.vcfxg_selftest_mfma_fp4(self.h, ctypes.byref(m)), "selftest")
        return m.value

    def text(self, nbytes):
        b = ctypes.create_string_buffer(max(1, nbytes))
        self._chk(self.L.vcfxg_fetch_text(self.h, b, nbytes), "fetch_text")
        return b.raw[:nbytes]

    def lines(self, n):
        import numpy as np
        alt = np.zeros(n, np.int32)
        tot = np.zeros(n, np.int32)
        st = np.zeros(n, np.uint8)
        self._chk(self.L.vcfxg_fetch_lines(self.h, 0, n, alt.ctypes.data, tot.ctypes.data, st.ctypes.data),
                  "fetch_lines")
        return alt, tot, st

    def statuses(self, n):
        """per-line status bytes of the last call (no counts)."""
        import numpy as np
        st = np.zeros(max(n, 1), np.uint8)
        self._chk(self.L.vcfxg_fetch_lines(self.h, 0, n, None, None, st.ctypes.data), "fetch_lines")
        return st[:n]

    def line_ends(self, n):
        import numpy as np
        out = np.zeros(n, np.uint64)
        self._chk(self.L.vcfxg_line_ends(self.h, 0, n, out.ctypes.data), "line_ends")
        return out


BGZF_MEMBER = None


def bgzf_members(buf):
    """The BGZF member table of buf (numpy uint8) for vcfxg_ingest_bgzf: every member a gzip
    member with FLG exactly FEXTRA and a 'BC' subfield (SAM/BAM spec §4.1), ISIZE <= 65536;
    raises ValueError otherwise (not a complete BGZF chain: the host inflates it)."""
    import numpy as np
    global BGZF_MEMBER
    if BGZF_MEMBER is None:
        BGZF_MEMBER = np.dtype([("src_off", "<u8"), ("src_len", "<u4"), ("out_len", "<u4")])
    b = bytes(buf) if not isinstance(buf, (bytes, bytearray)) else buf
    out, p, n = [], 0, len(b)
    while p < n:
        if n - p < 18 or b[p] != 0x1F or b[p + 1] != 0x8B or b[p + 2] != 8 or b[p + 3] != 4:
            raise ValueError("not a BGZF member at %d" % p)
        xlen = b[p + 10] | b[p + 11] << 8
        k, bs = 12, 0
        while k + 4 <= 12 + xlen and p + k + 4 <= n:
            slen = b[p + k + 2] | b[p + k + 3] << 8
            if b[p + k] == 66 and b[p + k + 1] == 67 and slen == 2:
                bs = (b[p + k + 4] | b[p + k + 5] << 8) + 1
            k += 4 + slen
        if not bs or p + bs > n or bs < 12 + xlen + 8:
            raise ValueError("bad BGZF member at %d" % p)
        isize = int.from_bytes(b[p + bs - 4:p + bs], "little")
        if isize > 65536:
            raise ValueError("ISIZE over 64 KiB at %d" % p)
        out.append((p, bs, isize))
        p += bs
    return np.array(out, dtype=BGZF_MEMBER)


def shard_cuts(buf, lo, world):
    """vcfxg_shard_cuts: world + 1 record-aligned cut offsets over [lo, len(buf)) (no device)"""
    import numpy as np
    arr = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
    cuts = np.zeros(world + 1, np.uint64)
    rc = lib().vcfxg_shard_cuts(arr.ctypes.data, arr.size, lo, world, cuts.ctypes.data)
    if rc != VCFXG_OK:
        raise EngineError("vcfxg_shard_cuts failed (%d)" % rc)
    return [int(x) for x in cuts]


def data_start_of(buf, strip_cr=True):
    """Byte offset just after the first '#CHROM' line (len(buf) if none)."""
    p = 0
    n = len(buf)
    while p < n:
        e = buf.find(b"\n", p)
        e = n if e < 0 else e
        line = buf[p:e]
        if strip_cr and line.endswith(b"\r"):
            line = line[:-1]
        nxt = e + 1 if e < n else n
        if line[:6] == b"#CHROM":
            return nxt
        p = nxt
    return n
