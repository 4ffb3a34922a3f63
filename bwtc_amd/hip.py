"""ctypes binding of libbwtc_hip.so (include/bwtc_hip.h).

This is the only way Python code in this repository reaches the GPU path.  There is no CPU
fallback: if the library is missing or a call fails, an exception is raised.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# BWTC_HIP_LIB: another build of the library (development: tile-shape sweeps, scripts/dev/)
LIB_PATH = os.environ.get("BWTC_HIP_LIB") or os.path.join(_HERE, "lib", "libbwtc_hip.so")

_vp = ctypes.c_void_p
_u32 = ctypes.c_uint32
_u64 = ctypes.c_uint64


class BwtcHipError(RuntimeError):
    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


# return codes of a corrupt 'H' record (bwtc_hip.h BWTC_HIP_E_*)
E_NO_CODE, E_SHAPE, E_PAST_RECORD, E_RUNS, E_CAPACITY, E_LENGTH = -10, -11, -12, -13, -14, -15


class HuffmanDecodeStats(ctypes.Structure):
    _fields_ = [("route", _u32), ("sections", _u32), ("streams", _u32), ("host_syncs", _u32),
                ("retries", _u32), ("max_code_len", _u32), ("runs", _u64), ("tiles", _u64), ("map_entries", _u64),
                ("launches", _u64), ("workspace_bytes", _u64), ("ms_entropy", ctypes.c_float),
                ("ms_entropy_wall", ctypes.c_float), ("ms_chain_host", ctypes.c_float), ("ms_inverse", ctypes.c_float)]


# return codes of the wavelet rebuild (bwtc_hip.h BWTC_HIP_E_W_*)
E_W_CHILD, E_W_BITS, E_W_ESCAPE, E_W_TOTAL, E_W_CAP, E_W_DEPTH, E_W_LIMIT, E_W_FOREST = -20, -21, -22, -23, -24, -25, -26, -27


class WaveletDecodeStats(ctypes.Structure):
    _fields_ = [("route", _u32), ("sections", _u32), ("routed_device", _u64), ("runs", _u64), ("nodes", _u64),
                ("words", _u64), ("bit_reads", _u64), ("launches", _u64), ("workspace_bytes", _u64),
                ("ms_range_decode", ctypes.c_float), ("ms_rebuild", ctypes.c_float), ("ms_inverse", ctypes.c_float)]


class WForestSection(ctypes.Structure):
    _fields_ = [(f, _u32) for f in ("runs", "bytes", "first_node", "symbol_nodes", "n_nodes", "first_code", "n_codes",
                                     "W", "plain_fixed")]


class WForestNode(ctypes.Structure):
    _fields_ = [("left", ctypes.c_int32), ("right", ctypes.c_int32), ("has_symbol", _u32), ("symbol", _u32),
                ("bits", _u32), ("first_word", _u32)]


class WForestCode(ctypes.Structure):
    _fields_ = [("left", ctypes.c_int32), ("right", ctypes.c_int32), ("has_symbol", _u32), ("symbol", _u32)]


class WForest(ctypes.Structure):
    _fields_ = [("sections", _vp), ("n_sections", _u32), ("nodes", _vp), ("n_nodes", _u32), ("codes", _vp),
                ("n_codes", _u32), ("words", _vp), ("n_words", _u64)]


SECTION_DTYPE = np.dtype([(f, np.uint32) for f, _ in WForestSection._fields_])
NODE_DTYPE = np.dtype([("left", np.int32), ("right", np.int32), ("has_symbol", np.uint32), ("symbol", np.uint32),
                       ("bits", np.uint32), ("first_word", np.uint32)])
CODE_DTYPE = np.dtype([("left", np.int32), ("right", np.int32), ("has_symbol", np.uint32), ("symbol", np.uint32)])


class Forest:
    """A flattened forest (bwtc_hip_wforest) over four numpy arrays: sections (SECTION_DTYPE), nodes (NODE_DTYPE),
    codes (CODE_DTYPE) and words (uint64)."""

    def __init__(self, sections, nodes, codes, words):
        self.sections = np.ascontiguousarray(sections, SECTION_DTYPE)
        self.nodes = np.ascontiguousarray(nodes, NODE_DTYPE)
        self.codes = np.ascontiguousarray(codes, CODE_DTYPE)
        self.words = np.ascontiguousarray(words, np.uint64)
        self.c = WForest(_ptr(self.sections), self.sections.size, _ptr(self.nodes), self.nodes.size,
                         _ptr(self.codes), self.codes.size, _ptr(self.words), self.words.size)

    @property
    def total(self):
        return int(self.sections["bytes"].astype(np.uint64).sum())


def host_wavelet_rebuild(forest, cap=None, line_words=7):
    """Host twin of the rebuild kernels (no device): forest -> (BWT bytes, bits taken out of nodes)."""
    cap = forest.total if cap is None else cap
    out = np.full(cap + 64, 0xA5, np.uint8)
    size, reads = _u64(0), _u64(0)
    _check(load().bwtc_hip_host_wavelet_rebuild(ctypes.byref(forest.c), _ptr(out), cap, ctypes.byref(size), line_words,
                                                ctypes.byref(reads)), "bwtc_hip_host_wavelet_rebuild")
    if not (out[cap:] == 0xA5).all():
        raise BwtcHipError("bytes past the capacity were modified")
    return out[:size.value].copy(), int(reads.value)


class WaveletDecoder:
    """The range decoder's state of one 'B' / 'b' / 'u' stream (bwtc_hip_wavelet_decoder): decode a stream's
    records in order through one of these."""

    def __init__(self, coder="B"):
        self.lib = load()
        self.h = self.lib.bwtc_hip_wavelet_decoder_create(coder.encode())
        if not self.h:
            raise BwtcHipError("bwtc_hip_wavelet_decoder_create('%s') failed" % coder)

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.bwtc_hip_wavelet_decoder_destroy(self.h)
            self.h = None

    def reset(self):
        self.lib.bwtc_hip_wavelet_decoder_reset(self.h)

    def decode_bwt_host(self, record, cap):
        """Pure host route: record -> (BWT bytes, LF powers, bytes consumed)."""
        record = np.ascontiguousarray(record, np.uint8)
        bwt = np.empty(max(cap, 1), np.uint8)
        lf = np.zeros(256, np.uint32)
        n_lf, size, used = _u32(0), _u32(0), _u64(0)
        _check(self.lib.bwtc_hip_wavelet_decode_bwt_host(self.h, _ptr(record), record.size, _ptr(bwt), cap, _ptr(lf),
                                                         ctypes.byref(n_lf), ctypes.byref(size), ctypes.byref(used)),
               "bwtc_hip_wavelet_decode_bwt_host")
        return bwt[:size.value].copy(), lf[:n_lf.value].copy(), int(used.value)

    def counts(self, record, cap):
        """Range-decodes the record and returns its forest's counts: dict(sections, runs, nodes, words, bytes,
        bit_reads), and the bytes consumed.  Moves the models on like any decode."""
        record = np.ascontiguousarray(record, np.uint8)
        c = np.zeros(6, np.uint64)
        used = _u64(0)
        _check(self.lib.bwtc_hip_wavelet_decode_counts(self.h, _ptr(record), record.size, cap, _ptr(c), ctypes.byref(used)),
               "bwtc_hip_wavelet_decode_counts")
        return dict(zip(("sections", "runs", "nodes", "words", "bytes", "bit_reads"), (int(v) for v in c))), int(used.value)


    def forest(self):
        """The forest of the last record decode_bwt_host / counts decoded, as the rebuild entry points take it, and
        its LF powers.  A view into the handle: use it before the handle's next call."""
        view = ForestView()
        lf = np.zeros(256, np.uint32)
        n_lf = _u32(0)
        _check(self.lib.bwtc_hip_wavelet_decoder_forest(self.h, ctypes.byref(view.c), _ptr(lf), ctypes.byref(n_lf)),
               "bwtc_hip_wavelet_decoder_forest")
        view.owner = self
        return view, lf[:n_lf.value].copy()


class ForestView:
    """A bwtc_hip_wforest that points into a WaveletDecoder handle (WaveletDecoder.forest)."""

    def __init__(self):
        self.c = WForest()
        self.owner = None

    @property
    def total(self):
        n = self.c.n_sections
        if n == 0:
            return 0
        secs = np.ctypeslib.as_array(ctypes.cast(self.c.sections, ctypes.POINTER(_u32)), (n, len(WForestSection._fields_)))
        return int(secs[:, 1].astype(np.uint64).sum())


class PostprocessStats(ctypes.Structure):
    _fields_ = [("route", _u32), ("launches", _u32), ("tokens", _u64), ("pair_tokens", _u64), ("in_bytes", _u64),
                ("out_bytes", _u64), ("pool_bytes", _u64), ("workspace_bytes", _u64), ("ms_device", ctypes.c_float)]


class Stats(ctypes.Structure):
    _fields_ = [("n", _u32), ("rounds", _u32), ("active_sum", _u64), ("sort_pass_items", _u64),
                ("ms_total", ctypes.c_float), ("ms_sort", ctypes.c_float),
                ("route", _u32), ("finisher_entries", _u32), ("alg_bytes", _u64)]


class WaveletRouteCounts(ctypes.Structure):
    _fields_ = [(f, _u64) for f in ("trees_device", "trees_host", "models_device", "models_rejected", "reject_reasons",
                                     "lost_turn", "models_host_two_stage", "models_host_fused", "models_host_lanes")]


# reasons a block's device models were not used (bwtc_hip.h BWTC_HIP_REJECT_*)
REJECT_FLAGS, REJECT_COUNT, REJECT_SCAN, REJECT_STATE, REJECT_TEST = 1, 2, 4, 8, 16


class FinPass(ctypes.Structure):
    """bwtc_hip_fin_pass (include/bwtc_hip.h): one k_finish launch of the finisher's test hooks."""
    _fields_ = [("n", _u32), ("nreg", _u32), ("ebase", _vp), ("ecount", _vp), ("S", _vp), ("P", _vp), ("H", _vp), ("C", _vp),
                ("window", ctypes.c_int), ("group", ctypes.c_int), ("words", ctypes.c_int), ("rounds", ctypes.c_int),
                ("floor", _u32), ("out_n", _u32), ("lf_n", _u32), ("lf_x", _u32), ("ranks", ctypes.c_int),
                ("rank", _vp), ("at", _u32), ("at2", _u32), ("us", _vp), ("ur", _vp), ("next_cap", _u32),
                ("nS", _vp), ("nP", _vp), ("nH", _vp), ("nC", _vp), ("next_base", _vp), ("next_count", _vp),
                ("hS", _vp), ("hHP", _vp), ("hC", _vp), ("hard_count", _vp), ("sS", _vp), ("sHP", _vp), ("shal_count", _vp),
                ("SA", _vp), ("out", _vp), ("small", _vp), ("lf", _vp)]


class FinRun(ctypes.Structure):
    """bwtc_hip_fin_run (include/bwtc_hip.h): the finisher's driver over a one-region list."""
    _fields_ = [("n", _u32), ("m", _u32), ("S", _vp), ("P", _vp), ("H", _vp), ("C", _vp),
                ("window", ctypes.c_int), ("group", ctypes.c_int), ("words", ctypes.c_int), ("rounds", ctypes.c_int),
                ("floor", _u32), ("out_n", _u32), ("lf_n", _u32), ("lf_x", _u32), ("keep_local", ctypes.c_int), ("max_passes", ctypes.c_int),
                ("outcome", _vp), ("info", _vp), ("pS", _vp), ("pHP", _vp), ("sS", _vp), ("sHP", _vp),
                ("lS", _vp), ("lP", _vp), ("lH", _vp), ("lC", _vp), ("SA", _vp), ("out", _vp), ("small", _vp), ("lf", _vp)]


class RankPass(ctypes.Structure):
    """bwtc_hip_rank_pass (include/bwtc_hip.h): one ranking through launch_rerank."""
    _fields_ = [("m", _u32), ("n", _u32)] + [(f, ctypes.c_int) for f in ("key_bytes", "init", "split", "lng", "mode", "emit")] + \
               [("keys", _vp), ("idx", _vp), ("w", _vp), ("aglob", _vp), ("short_len", _u32), ("kmask", _u64),
                ("wmask", _u32), ("hi_shift", ctypes.c_int), ("chr_shift", ctypes.c_int), ("chr_mask", _u32), ("lvl_shift", ctypes.c_int),
                ("depth", _u32), ("inv_lut", _vp), ("out_n", _u32), ("lf_n", _u32), ("lf_x", _u32), ("rec_shift", ctypes.c_int),
                ("plane", ctypes.c_int)] + \
               [(f, _vp) for f in ("aggA", "aggB", "aggC", "counts", "rank", "pair_s", "pair_r", "rec", "val", "rplane", "aidx", "aglob_out",
                                   "agrp", "achr", "SA", "out", "small", "lf")]


class RoundKeys(ctypes.Structure):
    """bwtc_hip_round_keys (include/bwtc_hip.h): one launch of a round's key kernel."""
    _fields_ = [("kind", ctypes.c_int), ("m", _u32), ("n", _u32), ("aidx", _vp), ("agrp", _vp), ("rec", _vp), ("val", _vp), ("rank", _vp),
                ("achr", _vp), ("h", _u32), ("bc", ctypes.c_int), ("emit", ctypes.c_int), ("bin_shift", ctypes.c_int), ("run_mode", ctypes.c_int),
                ("k", _vp), ("h_split", _u32), ("p", _u32), ("keys", _vp)]


class Round(ctypes.Structure):
    """bwtc_hip_round (include/bwtc_hip.h): rank_step<u64, false> once."""
    _fields_ = [("m", _u32), ("n", _u32), ("ks", _vp), ("vs", _vp), ("aglob", _vp), ("rank", _vp), ("k", _vp), ("h_next", _u64)] + \
               [(f, ctypes.c_int) for f in ("emit", "text", "carry_in", "raw_out", "run_mode")] + \
               [("step_p", _u32), ("step_depth", _u32), ("pairs_min", _u32), ("window_bits", ctypes.c_int), ("out_n", _u32), ("lf_n", _u32),
                ("lf_x", _u32)] + [(f, _vp) for f in ("result", "nks", "nvs", "naglob", "ngrp", "nchr", "SA", "out", "small", "lf")]


class ModelsOut(ctypes.Structure):
    """bwtc_hip_models_out (include/bwtc_hip.h): what the model passes left, copied back by bwtc_hip_test_models."""
    _fields_ = [("w", _vp), ("tail", _u32 * 4), ("ends", _u32 * 8), ("nc", _u32), ("nsc", _u32)] + \
               [(f, _vp) for f in ("chunks", "cmap", "cstate", "base", "sb", "sbits", "smap", "snaps", "sstart")]


class BatchItem(ctypes.Structure):
    """bwtc_hip_batch_item: one block of a batched transform."""
    _fields_ = [("offset", _u64), ("size", _u32), ("n_lf", _u32)]


class BatchStats(ctypes.Structure):
    """bwtc_hip_batch_stats: what the last batched transform on a context did."""
    _fields_ = [("blocks", _u32), ("stride_log2", _u32), ("rounds", _u32), ("host_waits", _u32), ("suffixes", _u64),
                ("active", _u64 * 32), ("ms_total", ctypes.c_float)]


class KernelTimers(ctypes.Structure):
    _fields_ = [("scatter_launches", _u64), ("scatter_bytes", _u64), ("scatter_ms", ctypes.c_double)]


# the C ABI's lowercase names (bwtc_hip_decode_block_H and bwtc_hip_decode_block_W[_device|_begin|_end|_end_device] are exported too;
# tests/test_huffman_decode_abi.py and tests/test_wavelet_rebuild_host.py check them)
EXPORTS = [
    "bwtc_hip_huffman_decode", "bwtc_hip_huffman_decode_device", "bwtc_hip_huffman_decode_stats_get",
    "bwtc_hip_device_count", "bwtc_hip_version", "bwtc_hip_workspace_bytes", "bwtc_hip_create",
    "bwtc_hip_destroy", "bwtc_hip_stream", "bwtc_hip_get_stats", "bwtc_hip_set_profiling",
    "bwtc_hip_get_kernel_timers", "bwtc_hip_copy_probe", "bwtc_hip_test_gpu_lanes", "bwtc_hip_malloc", "bwtc_hip_free", "bwtc_hip_memcpy_to_device",
    "bwtc_hip_memcpy_to_host", "bwtc_hip_host_alloc", "bwtc_hip_host_free",
    "bwtc_hip_memcpy_to_device_async", "bwtc_hip_copy_wait", "bwtc_hip_wavelet_host_clock", "bwtc_hip_wavelet_host_progress", "bwtc_hip_wavelet_latency", "bwtc_hip_wavelet_routes", "bwtc_hip_host_staging_bytes", "bwtc_hip_host_usable_cpus", "bwtc_hip_n_lf", "bwtc_hip_bwt",
    "bwtc_hip_bwt_block", "bwtc_hip_bwt_block_device", "bwtc_hip_inverse_bwt_block",
    "bwtc_hip_bwt_blocks", "bwtc_hip_bwt_blocks_device", "bwtc_hip_batch_stats_get", "bwtc_hip_test_batch_keys",
    "bwtc_hip_inverse_bwt_block_device", "bwtc_hip_compress_bound",
    "bwtc_hip_huffman_encode_device", "bwtc_hip_huffman_encode", "bwtc_hip_transform_and_encode",
    "bwtc_hip_wavelet_section_stats", "bwtc_hip_transform_and_encode_wavelet", "bwtc_hip_wavelet_encode",
    "bwtc_hip_wavelet_encode_device", "bwtc_hip_wavelet_encode_device_begin", "bwtc_hip_wavelet_encode_end",
    "bwtc_hip_wavelet_encode_device_prepare", "bwtc_hip_wavelet_encode_queue",
    "bwtc_hip_wavelet_depth", "bwtc_hip_wavelet_set_depth", "bwtc_hip_numa_node", "bwtc_hip_host_cpu_slice", "bwtc_hip_set_worker_cpus", "bwtc_hip_wavelet_reset", "bwtc_hip_wavelet_start", "bwtc_hip_host_wavelet_sections", "bwtc_hip_host_wavelet_streams", "bwtc_hip_host_wavelet_streams_lanes", "bwtc_hip_host_huffman_lengths", "bwtc_hip_host_huffman_codes", "bwtc_hip_host_serialize_shape",
    "bwtc_hip_host_sections", "bwtc_hip_host_bwtblock_header", "bwtc_hip_synth", "bwtc_hip_suffix_array",
    "bwtc_hip_test_sort_u32", "bwtc_hip_test_sort_u64", "bwtc_hip_test_scan_u32",
    "bwtc_hip_test_radix_pairs", "bwtc_hip_test_radix_long", "bwtc_hip_test_radix_segmented",
    "bwtc_hip_period_get", "bwtc_hip_test_period_lengths", "bwtc_hip_steps_get", "bwtc_hip_test_period_proper",
    "bwtc_hip_test_period_merge", "bwtc_hip_test_period_winners", "bwtc_hip_schedule_get",
    "bwtc_hip_copies_get", "bwtc_hip_test_copy_lengths",
    "bwtc_hip_test_long_period_votes", "bwtc_hip_test_long_period_probe", "bwtc_hip_test_long_period_lengths",
    "bwtc_hip_test_code_stage", "bwtc_hip_test_code_table", "bwtc_hip_test_code_keys",
    "bwtc_hip_test_finish_pass", "bwtc_hip_test_local_pass", "bwtc_hip_test_finisher",
    "bwtc_hip_test_models", "bwtc_hip_host_test_models", "bwtc_hip_host_wavelet_elements",
    "bwtc_hip_test_models_letter", "bwtc_hip_host_test_models_letter", "bwtc_hip_host_wavelet_elements_letter",
    "bwtc_hip_test_rank_pass", "bwtc_hip_test_rank_scan", "bwtc_hip_test_rank_scatter", "bwtc_hip_test_round_keys", "bwtc_hip_test_round",
    "bwtc_hip_wavelet_depth_needed", "bwtc_hip_grammar_create", "bwtc_hip_grammar_destroy", "bwtc_hip_grammar_rules", "bwtc_hip_grammar_special_symbols",
    "bwtc_hip_grammar_is_special", "bwtc_hip_grammar_write", "bwtc_hip_grammar_read", "bwtc_hip_pair_replace_device",
    "bwtc_hip_test_pair_stats", "bwtc_hip_precompress", "bwtc_hip_host_precompress", "bwtc_hip_postprocess",
    "bwtc_hip_postprocess_device", "bwtc_hip_postprocess_block", "bwtc_hip_postprocess_stats_get",
    "bwtc_hip_host_postprocess_tiles",
    "bwtc_hip_wavelet_decoder_create", "bwtc_hip_wavelet_decoder_destroy", "bwtc_hip_wavelet_decoder_reset",
    "bwtc_hip_wavelet_decode_bwt_host",
    "bwtc_hip_wavelet_decode_counts", "bwtc_hip_wavelet_decoder_forest", "bwtc_hip_wavelet_rebuild", "bwtc_hip_wavelet_rebuild_device",
    "bwtc_hip_host_wavelet_rebuild", "bwtc_hip_wavelet_decode_stats_get",
]

_lib = None


def load():
    """Load libbwtc_hip.so; raises BwtcHipError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BwtcHipError(
            "%s not found: build it with `make -C bwtc_amd/csrc` (or __graft_entry__.build()); "
            "there is no CPU fallback" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    L.bwtc_hip_device_count.restype = ctypes.c_int
    L.bwtc_hip_version.restype = ctypes.c_char_p
    L.bwtc_hip_workspace_bytes.restype = _u64
    L.bwtc_hip_workspace_bytes.argtypes = [_u32]
    L.bwtc_hip_create.argtypes = [ctypes.c_int, _u32, ctypes.POINTER(_vp)]
    L.bwtc_hip_destroy.argtypes = [_vp]
    L.bwtc_hip_destroy.restype = None
    L.bwtc_hip_stream.restype = _vp
    L.bwtc_hip_stream.argtypes = [_vp]
    L.bwtc_hip_get_stats.argtypes = [_vp, ctypes.POINTER(Stats)]
    L.bwtc_hip_set_profiling.argtypes = [_vp, ctypes.c_int]
    L.bwtc_hip_get_kernel_timers.argtypes = [_vp, ctypes.POINTER(KernelTimers), ctypes.c_int]
    L.bwtc_hip_test_gpu_lanes.argtypes = [_vp, _vp, _u64, _vp, _u32, ctypes.c_int, _vp, _u64, _vp]
    L.bwtc_hip_copy_probe.argtypes = [_vp, _u64, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    L.bwtc_hip_malloc.restype = _vp
    L.bwtc_hip_malloc.argtypes = [_vp, _u64]
    L.bwtc_hip_free.restype = None
    L.bwtc_hip_free.argtypes = [_vp, _vp]
    L.bwtc_hip_memcpy_to_device.argtypes = [_vp, _vp, _vp, _u64]
    L.bwtc_hip_memcpy_to_host.argtypes = [_vp, _vp, _vp, _u64]
    L.bwtc_hip_host_alloc.restype = _vp
    L.bwtc_hip_host_alloc.argtypes = [_vp, _u64]
    L.bwtc_hip_host_free.restype = None
    L.bwtc_hip_host_free.argtypes = [_vp, _vp]
    L.bwtc_hip_memcpy_to_device_async.argtypes = [_vp, _vp, _vp, _u64]
    L.bwtc_hip_copy_wait.argtypes = [_vp]
    L.bwtc_hip_wavelet_host_clock.argtypes = [_vp, _vp, _vp, _vp]
    L.bwtc_hip_wavelet_host_progress.argtypes = [_vp, _vp, _vp]
    L.bwtc_hip_wavelet_latency.argtypes = [_vp, _vp]
    L.bwtc_hip_wavelet_routes.argtypes = [_vp, _vp, ctypes.c_int]
    L.bwtc_hip_host_staging_bytes.argtypes = [_vp, _vp]
    L.bwtc_hip_numa_node.argtypes = [_vp]
    L.bwtc_hip_host_cpu_slice.argtypes = [ctypes.c_int, _u32, _u32, _vp, _u32]
    L.bwtc_hip_set_worker_cpus.argtypes = [_vp, _vp, _u32]
    L.bwtc_hip_synth.argtypes = [ctypes.c_char, _u64, _u64, _vp]
    L.bwtc_hip_n_lf.restype = _u32
    L.bwtc_hip_n_lf.argtypes = [_u32, _u32]
    L.bwtc_hip_bwt.argtypes = [_vp, _vp, _u32, _vp, _u32, _vp]
    L.bwtc_hip_bwt_block.argtypes = [_vp, _vp, _u32, _vp, _u32, _vp]
    L.bwtc_hip_bwt_block_device.argtypes = [_vp, _vp, _vp, _u32, _vp, _u32, _vp]
    L.bwtc_hip_bwt_blocks.argtypes = [_vp, _vp, _vp, _u32, _vp, _vp]
    L.bwtc_hip_bwt_blocks_device.argtypes = [_vp, _vp, _vp, _vp, _u32, _vp, _vp]
    L.bwtc_hip_batch_stats_get.argtypes = [_vp, ctypes.POINTER(BatchStats)]
    L.bwtc_hip_test_batch_keys.argtypes = [_vp, _vp, _vp, _u32, _vp, _vp, _vp]
    L.bwtc_hip_inverse_bwt_block.argtypes = [_vp, _vp, _u32, _vp, _u32]
    L.bwtc_hip_inverse_bwt_block_device.argtypes = [_vp, _vp, _vp, _u32, _vp, _u32]
    L.bwtc_hip_compress_bound.restype = _u64
    L.bwtc_hip_compress_bound.argtypes = [_u32]
    L.bwtc_hip_huffman_encode_device.argtypes = [_vp, _vp, _u32, _vp, _u32, _vp, _vp, _u64,
                                                 ctypes.POINTER(_u64)]
    L.bwtc_hip_huffman_encode.argtypes = [_vp, _vp, _u32, _vp, _u32, _vp, _vp, _u64,
                                          ctypes.POINTER(_u64)]
    L.bwtc_hip_huffman_decode.argtypes = [_vp, _vp, _u64, _vp, _u64, _vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32),
                                          ctypes.POINTER(_u64)]
    L.bwtc_hip_huffman_decode_device.argtypes = L.bwtc_hip_huffman_decode.argtypes
    L.bwtc_hip_decode_block_H.argtypes = [_vp, _vp, _u64, _vp, _u64, ctypes.POINTER(_u32), ctypes.POINTER(_u64)]
    L.bwtc_hip_huffman_decode_stats_get.argtypes = [_vp, ctypes.POINTER(HuffmanDecodeStats)]
    L.bwtc_hip_transform_and_encode.argtypes = [_vp, _vp, _u32, _u32, _vp, _u64, ctypes.POINTER(_u64)]
    L.bwtc_hip_wavelet_section_stats.argtypes = [_vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32]
    L.bwtc_hip_transform_and_encode_wavelet.argtypes = [_vp, _vp, _u32, _u32, _u32, _vp, _u64, ctypes.POINTER(_u64)]
    L.bwtc_hip_wavelet_encode.argtypes = [_vp, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u64, ctypes.POINTER(_u64)]
    L.bwtc_hip_wavelet_encode_device.argtypes = [_vp, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u64, ctypes.POINTER(_u64)]
    L.bwtc_hip_wavelet_encode_device_begin.argtypes = [_vp, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u64, ctypes.POINTER(_u64)]
    L.bwtc_hip_wavelet_encode_end.argtypes = [_vp, _u64, ctypes.POINTER(_u64)]
    L.bwtc_hip_wavelet_encode_device_prepare.argtypes = [_vp, _vp, _u32, _vp, _u32, _vp, _u32, _vp, _u64, ctypes.POINTER(_u64)]
    L.bwtc_hip_wavelet_encode_queue.argtypes = [_vp, _u64, _u32, ctypes.POINTER(_u32)]
    L.bwtc_hip_wavelet_depth.restype = ctypes.c_uint32
    L.bwtc_hip_wavelet_depth.argtypes = [_vp]
    L.bwtc_hip_wavelet_set_depth.argtypes = [_vp, ctypes.c_uint32]
    L.bwtc_hip_wavelet_depth_needed.restype = ctypes.c_uint32
    L.bwtc_hip_wavelet_depth_needed.argtypes = [_vp]
    L.bwtc_hip_wavelet_reset.restype = None
    L.bwtc_hip_wavelet_reset.argtypes = [_vp]
    L.bwtc_hip_wavelet_start.argtypes = [_vp, ctypes.c_char]
    L.bwtc_hip_host_wavelet_sections.argtypes = [_u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u32, ctypes.c_char, _vp, _vp, _u64,
                                                 ctypes.POINTER(_u64)]
    L.bwtc_hip_host_wavelet_streams.argtypes = L.bwtc_hip_host_wavelet_sections.argtypes
    L.bwtc_hip_test_models.argtypes = [_vp, _vp, _u32, _vp, _u32, _u32, _u32, ctypes.POINTER(ModelsOut)]
    L.bwtc_hip_host_test_models.argtypes = [_vp, _u32, _vp, _u32, _u32, _vp, ctypes.POINTER(_u32)]
    L.bwtc_hip_test_models_letter.argtypes = [_vp, ctypes.c_char, _vp, _u32, _vp, _u32, _u32, _u32, ctypes.POINTER(ModelsOut)]
    L.bwtc_hip_host_test_models_letter.argtypes = [ctypes.c_char, _vp, _u32, _vp, _u32, _u32, _vp, ctypes.POINTER(_u32)]
    L.bwtc_hip_host_wavelet_elements.argtypes = [_u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32),
                                                 ctypes.POINTER(_u32), _vp, _u64, _vp, _u32, _vp, _u64]
    L.bwtc_hip_host_wavelet_elements_letter.argtypes = [ctypes.c_char] + L.bwtc_hip_host_wavelet_elements.argtypes
    L.bwtc_hip_host_wavelet_streams_lanes.argtypes = L.bwtc_hip_host_wavelet_sections.argtypes
    # pair-replacing pre-stage (`--prepr`)
    L.bwtc_hip_grammar_create.restype = _vp
    L.bwtc_hip_grammar_create.argtypes = []
    L.bwtc_hip_grammar_destroy.restype = None
    L.bwtc_hip_grammar_destroy.argtypes = [_vp]
    L.bwtc_hip_grammar_rules.restype = _u32
    L.bwtc_hip_grammar_rules.argtypes = [_vp]
    L.bwtc_hip_grammar_special_symbols.restype = _u32
    L.bwtc_hip_grammar_special_symbols.argtypes = [_vp]
    L.bwtc_hip_grammar_is_special.argtypes = [_vp, ctypes.c_uint]
    L.bwtc_hip_grammar_write.argtypes = [_vp, _vp, _u64, ctypes.POINTER(_u64)]
    L.bwtc_hip_grammar_read.argtypes = [_vp, _vp, _u64, ctypes.POINTER(_u64)]
    L.bwtc_hip_pair_replace_device.argtypes = [_vp, _vp, _vp, _u64, _vp, ctypes.POINTER(_u64), ctypes.POINTER(_u32)]
    L.bwtc_hip_test_pair_stats.argtypes = [_vp, _vp, _u64, _vp, _vp]
    L.bwtc_hip_precompress.argtypes = [_vp, _vp, ctypes.c_char_p, _vp, _u64, ctypes.POINTER(_u64)]
    L.bwtc_hip_host_precompress.argtypes = [_vp, ctypes.c_char_p, _vp, _u64, ctypes.POINTER(_u64)]
    L.bwtc_hip_postprocess.argtypes = [_vp, _vp, _u64, _vp, _u64, ctypes.POINTER(_u64)]
    L.bwtc_hip_postprocess_device.argtypes = [_vp, _vp, _vp, _u64, _vp, _u64, ctypes.POINTER(_u64)]
    L.bwtc_hip_postprocess_block.argtypes = [_vp, _vp, _vp, _u64, _vp, _u64, ctypes.POINTER(_u64)]
    L.bwtc_hip_postprocess_stats_get.argtypes = [_vp, ctypes.POINTER(PostprocessStats)]
    L.bwtc_hip_host_postprocess_tiles.argtypes = [_vp, _vp, _u64, _vp, _u64, ctypes.POINTER(_u64), _u32]
    L.bwtc_hip_decode_block_H_device.argtypes = [_vp, _vp, _u64, _vp, _u64, ctypes.POINTER(_u32), ctypes.POINTER(_u64)]
    L.bwtc_hip_wavelet_decoder_create.restype = _vp
    L.bwtc_hip_wavelet_decoder_create.argtypes = [ctypes.c_char]
    L.bwtc_hip_wavelet_decoder_destroy.restype = None
    L.bwtc_hip_wavelet_decoder_destroy.argtypes = [_vp]
    L.bwtc_hip_wavelet_decoder_reset.restype = None
    L.bwtc_hip_wavelet_decoder_reset.argtypes = [_vp]
    L.bwtc_hip_decode_block_W.argtypes = [_vp, _vp, _vp, _u64, _vp, _u64, ctypes.POINTER(_u32), ctypes.POINTER(_u64)]
    L.bwtc_hip_decode_block_W_device.argtypes = L.bwtc_hip_decode_block_W.argtypes
    L.bwtc_hip_decode_block_W_begin.argtypes = [_vp, _vp, _vp, _u64, _u64, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u64)]
    L.bwtc_hip_decode_block_W_end.argtypes = [_vp, _u32, _vp, _u64, ctypes.POINTER(_u32)]
    L.bwtc_hip_decode_block_W_end_device.argtypes = L.bwtc_hip_decode_block_W_end.argtypes
    L.bwtc_hip_wavelet_decode_bwt_host.argtypes = [_vp, _vp, _u64, _vp, _u64, _vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32),
                                                   ctypes.POINTER(_u64)]
    L.bwtc_hip_wavelet_decode_counts.argtypes = [_vp, _vp, _u64, _u64, _vp, ctypes.POINTER(_u64)]
    L.bwtc_hip_wavelet_decoder_forest.argtypes = [_vp, ctypes.POINTER(WForest), _vp, ctypes.POINTER(_u32)]
    L.bwtc_hip_wavelet_rebuild.argtypes = [_vp, ctypes.POINTER(WForest), _vp, _u64, ctypes.POINTER(_u64)]
    L.bwtc_hip_wavelet_rebuild_device.argtypes = L.bwtc_hip_wavelet_rebuild.argtypes
    L.bwtc_hip_host_wavelet_rebuild.argtypes = [ctypes.POINTER(WForest), _vp, _u64, ctypes.POINTER(_u64), _u32, ctypes.POINTER(_u64)]
    L.bwtc_hip_wavelet_decode_stats_get.argtypes = [_vp, ctypes.POINTER(WaveletDecodeStats)]
    L.bwtc_hip_host_huffman_lengths.restype = None
    L.bwtc_hip_host_huffman_lengths.argtypes = [_vp, _vp]
    L.bwtc_hip_host_huffman_codes.restype = None
    L.bwtc_hip_host_huffman_codes.argtypes = [_vp, _vp]
    L.bwtc_hip_host_serialize_shape.restype = _u32
    L.bwtc_hip_host_serialize_shape.argtypes = [_vp, _vp, _u32]
    L.bwtc_hip_host_sections.restype = _u32
    L.bwtc_hip_host_sections.argtypes = [_vp, _vp]
    L.bwtc_hip_host_bwtblock_header.restype = _u32
    L.bwtc_hip_host_bwtblock_header.argtypes = [_vp, _u32, _vp, _u32]
    L.bwtc_hip_suffix_array.argtypes = [_vp, _vp, _u32, _vp]
    L.bwtc_hip_test_sort_u32.argtypes = [_vp, _vp, _vp, _u64, ctypes.c_int]
    L.bwtc_hip_test_sort_u64.argtypes = [_vp, _vp, _vp, _u64, ctypes.c_int]
    L.bwtc_hip_test_scan_u32.argtypes = [_vp, _vp, _u64]
    L.bwtc_hip_test_radix_pairs.argtypes = [_vp, _vp, _vp, _u64, _u64] + [ctypes.c_int] * 6
    L.bwtc_hip_test_radix_long.argtypes = [_vp, _vp, _vp, _vp, _u64] + [ctypes.c_int] * 5
    L.bwtc_hip_test_radix_segmented.argtypes = [_vp, _vp, _u64, ctypes.c_int, _vp, _u32]
    L.bwtc_hip_period_get.argtypes = [_vp] + [ctypes.POINTER(_u32)] * 4
    L.bwtc_hip_test_period_lengths.argtypes = [_vp, _vp, _u32, _u32, _vp, ctypes.POINTER(_u32)]
    L.bwtc_hip_steps_get.argtypes = [_vp] + [ctypes.POINTER(_u32)] * 5
    L.bwtc_hip_test_period_proper.argtypes = [_vp, _vp, _u32, _u32, _vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32)]
    L.bwtc_hip_test_period_merge.argtypes = [_vp, _vp, _u32, _u32, _u32, ctypes.c_int, _vp, ctypes.POINTER(_u32), ctypes.POINTER(_u32)]
    L.bwtc_hip_schedule_get.argtypes = [_vp, _vp, _u32, ctypes.POINTER(_u32)]
    L.bwtc_hip_copies_get.argtypes = [_vp] + [ctypes.POINTER(_u32)] * 4
    L.bwtc_hip_test_copy_lengths.argtypes = [_vp, _vp, _vp, _u32, _vp, _u32, _vp, ctypes.POINTER(_u32)]
    L.bwtc_hip_test_period_winners.argtypes = [_vp, _vp, _u32, _vp, ctypes.POINTER(_u32)]
    L.bwtc_hip_test_long_period_votes.argtypes = [_vp, _vp, _vp, _u32, _u64, _vp, _u32, _vp, ctypes.POINTER(_u32)]
    L.bwtc_hip_test_long_period_probe.argtypes = [_vp, _vp, _u32, _u32, _u32, ctypes.POINTER(_u32)]
    L.bwtc_hip_test_long_period_lengths.argtypes = [_vp, _vp, _u32, _u32, _vp, _vp]
    L.bwtc_hip_test_code_stage.argtypes = [_vp, _vp, _u32, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, ctypes.POINTER(_u32), _vp, _vp,
                                           ctypes.POINTER(_u32), _vp, _vp, _vp]
    L.bwtc_hip_test_code_table.argtypes = [_vp, _vp, _u32, _vp, ctypes.POINTER(_u32)]
    L.bwtc_hip_test_code_keys.argtypes = [_vp, _vp, _u32, ctypes.c_int, ctypes.c_int, _vp, _u32, _vp, _vp, _vp, _vp]
    L.bwtc_hip_test_finish_pass.argtypes = [_vp, _vp, ctypes.POINTER(FinPass)]
    L.bwtc_hip_test_local_pass.argtypes = [_vp, _vp, ctypes.POINTER(FinPass)]
    L.bwtc_hip_test_finisher.argtypes = [_vp, _vp, ctypes.POINTER(FinRun)]
    L.bwtc_hip_test_rank_pass.argtypes = [_vp, _vp, ctypes.POINTER(RankPass)]
    L.bwtc_hip_test_rank_scan.argtypes = [_vp, _vp, _vp, _vp, _u32, _vp, _u32, _vp]
    L.bwtc_hip_test_rank_scatter.argtypes = [_vp, ctypes.c_int, _vp, _vp, _vp, _u32, _u32, ctypes.c_int, _vp]
    L.bwtc_hip_test_round_keys.argtypes = [_vp, _vp, ctypes.POINTER(RoundKeys)]
    L.bwtc_hip_test_round.argtypes = [_vp, _vp, ctypes.POINTER(Round)]
    _lib = L
    return L


def _check(rc, what):
    if rc != 0:
        raise BwtcHipError("%s failed with code %d" % (what, rc), rc)


def _ptr(a):
    return a.ctypes.data_as(_vp)


class Grammar:
    """bwtc::Grammar of one precompressor block (bwtc_hip_grammar): what the `--prepr` rounds did to it."""

    def __init__(self):
        self.lib = load()
        self.h = self.lib.bwtc_hip_grammar_create()
        if not self.h:
            raise BwtcHipError("bwtc_hip_grammar_create failed")

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.bwtc_hip_grammar_destroy(self.h)
            self.h = None

    @property
    def rules(self):
        return int(self.lib.bwtc_hip_grammar_rules(self.h))

    @property
    def special_symbols(self):
        return int(self.lib.bwtc_hip_grammar_special_symbols(self.h))

    def is_special(self, c):
        return bool(self.lib.bwtc_hip_grammar_is_special(self.h, int(c)))

    def write(self):
        out = np.zeros((1 << 17) + 8 * self.rules, np.uint8)      # a rule costs at most seven bytes, the freed symbols' table at most 64 KiB
        n = _u64(0)
        _check(self.lib.bwtc_hip_grammar_write(self.h, _ptr(out), out.size, ctypes.byref(n)), "bwtc_hip_grammar_write")
        return out[:n.value].copy()

    def read(self, raw):
        raw = np.ascontiguousarray(raw, np.uint8)
        n = _u64(0)
        _check(self.lib.bwtc_hip_grammar_read(self.h, _ptr(raw), raw.size, ctypes.byref(n)), "bwtc_hip_grammar_read")
        return int(n.value)

    def host_precompress(self, options, data):
        """Precompressor::precompress with both sweeps on the calling thread (no device)."""
        buf = np.ascontiguousarray(data, np.uint8).copy()
        n = _u64(0)
        _check(self.lib.bwtc_hip_host_precompress(self.h, options.encode(), _ptr(buf), buf.size, ctypes.byref(n)), "bwtc_hip_host_precompress")
        return buf[:n.value].copy()

    def postprocess(self, data, max_size):
        data = np.ascontiguousarray(data, np.uint8)
        out = np.zeros(max(1, max_size), np.uint8)
        n = _u64(0)
        _check(self.lib.bwtc_hip_postprocess(self.h, _ptr(data), data.size, _ptr(out), out.size, ctypes.byref(n)), "bwtc_hip_postprocess")
        return out[:n.value].copy()

    def host_postprocess_tiles(self, data, max_size, tile):
        """Host twin of the device postprocessor's passes over tiles of `tile` bytes (no device)."""
        data = np.ascontiguousarray(data, np.uint8)
        out = np.zeros(max(1, max_size), np.uint8)
        n = _u64(0)
        _check(self.lib.bwtc_hip_host_postprocess_tiles(self.h, _ptr(data), data.size, _ptr(out), max_size, ctypes.byref(n), tile),
               "bwtc_hip_host_postprocess_tiles")
        return out[:n.value].copy()


class Context:
    """One GPU, one stream, one persistent workspace (bwtc_hip_ctx)."""

    def __init__(self, device=0, max_block_size=1 << 20):
        self.lib = load()
        if self.lib.bwtc_hip_device_count() <= 0:
            raise BwtcHipError("no HIP device visible")
        h = _vp()
        _check(self.lib.bwtc_hip_create(device, max_block_size, ctypes.byref(h)), "bwtc_hip_create")
        self.handle = h
        self.max_block_size = max_block_size

    def close(self):
        if getattr(self, "handle", None):
            self.lib.bwtc_hip_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def n_lf(self, size, starting_points):
        return int(self.lib.bwtc_hip_n_lf(size, starting_points))

    def precompress(self, grammar, options, data):
        """Precompressor::precompress on the GPU (bwtc_hip_precompress): the precompressed block."""
        buf = np.ascontiguousarray(data, np.uint8).copy()
        n = _u64(0)
        _check(self.lib.bwtc_hip_precompress(self.handle, grammar.h, options.encode(), _ptr(buf), buf.size, ctypes.byref(n)), "bwtc_hip_precompress")
        return buf[:n.value].copy()

    def pair_replace_device(self, grammar, d_src_ptr, n, d_dst_ptr):
        """One PairReplacer round on device pointers (bwtc_hip_pair_replace_device; d_dst: room for 2 n bytes):
        (new length, pairs replaced)."""
        n_out, replaced = _u64(0), _u32(0)
        _check(self.lib.bwtc_hip_pair_replace_device(self.handle, grammar.h, _vp(d_src_ptr), n, _vp(d_dst_ptr), ctypes.byref(n_out),
                                                     ctypes.byref(replaced)), "bwtc_hip_pair_replace_device")
        return int(n_out.value), int(replaced.value)

    def test_pair_stats(self, d_ptr, n):
        """The statistics step of a round alone (bwtc_hip_test_pair_stats) over n device bytes at d_ptr:
        (byte counters[256], pair counters[65536], index = first << 8 | second)."""
        pair_cnt = np.zeros(65536, np.uint32)
        byte_cnt = np.zeros(256, np.uint32)
        _check(self.lib.bwtc_hip_test_pair_stats(self.handle, _vp(d_ptr), n, _ptr(pair_cnt), _ptr(byte_cnt)), "bwtc_hip_test_pair_stats")
        return byte_cnt, pair_cnt

    def postprocess(self, grammar, data, max_size):
        """Postprocessor::uncompress on the GPU (bwtc_hip_postprocess_block): host buffers in and out."""
        data = np.ascontiguousarray(data, np.uint8)
        out = np.zeros(max(1, max_size), np.uint8)
        n = _u64(0)
        _check(self.lib.bwtc_hip_postprocess_block(self.handle, grammar.h, _ptr(data), data.size, _ptr(out), max_size, ctypes.byref(n)),
               "bwtc_hip_postprocess_block")
        return out[:n.value].copy()

    def postprocess_device(self, grammar, d_data_ptr, n, d_out_ptr, cap):
        """The same on device pointers (bwtc_hip_postprocess_device): the expansion's size."""
        n_out = _u64(0)
        _check(self.lib.bwtc_hip_postprocess_device(self.handle, grammar.h, _vp(d_data_ptr), n, _vp(d_out_ptr), cap, ctypes.byref(n_out)),
               "bwtc_hip_postprocess_device")
        return int(n_out.value)

    def postprocess_stats(self):
        s = PostprocessStats()
        _check(self.lib.bwtc_hip_postprocess_stats_get(self.handle, ctypes.byref(s)), "bwtc_hip_postprocess_stats_get")
        return {f: getattr(s, f) for f, _ in PostprocessStats._fields_}

    def stats(self):
        s = Stats()
        _check(self.lib.bwtc_hip_get_stats(self.handle, ctypes.byref(s)), "bwtc_hip_get_stats")
        return s

    def reset_kernel_timers(self):
        """Turns per-kernel event timing on and clears the accumulators."""
        _check(self.lib.bwtc_hip_set_profiling(self.handle, 1), "bwtc_hip_set_profiling")
        _check(self.lib.bwtc_hip_get_kernel_timers(self.handle, None, 1), "bwtc_hip_get_kernel_timers")

    def kernel_timers(self):
        k = KernelTimers()
        _check(self.lib.bwtc_hip_get_kernel_timers(self.handle, ctypes.byref(k), 0),
               "bwtc_hip_get_kernel_timers")
        return {"scatter_launches": int(k.scatter_launches), "scatter_bytes": int(k.scatter_bytes),
                "scatter_ms": float(k.scatter_ms)}

    def test_gpu_lanes(self, w, bounds, mode=0):
        """Chains of w-elements through the GPU lane engine (mode 0) or the host's scalar coder (mode 1): list of byte strings."""
        w = np.ascontiguousarray(w, np.uint16)
        b = np.ascontiguousarray(bounds, np.uint64)
        k = b.size - 1
        out = np.zeros(int(w.size) * 4 + 16 * k + 64, np.uint8)
        off = np.zeros(k + 1, np.uint64)
        _check(self.lib.bwtc_hip_test_gpu_lanes(self.handle, _ptr(w), w.size, _ptr(b), k, mode, _ptr(out), out.size, _ptr(off)),
               "bwtc_hip_test_gpu_lanes")
        return [out[int(off[j]):int(off[j + 1])].tobytes() for j in range(k)]

    def test_models(self, packed, n_coded, tasks, state_in, flags=0, letter="B"):
        """The model passes (wavelet_gpu_models.hip) over given packed streams and tasks [(begin, end, type)]: a dict of
        w, tail, ends, nc, nsc and -- unless flags bit 1 -- chunks, cmap, cstate, base, sb, sbits, smap, snaps, sstart.
        flags bit 0: the lines form of the partition pass (bwtc_hip_test_models); letter: the main model
        (bwtc_hip_test_models_letter for 'b' and 'u')."""
        packed, tasks = _models_args(packed, tasks)
        nt, n = tasks.shape[0], int(n_coded)
        nc_room, nsc = nt + n // 2048, (n + 2047) // 2048
        r = {"w": np.zeros(n, np.uint16)}
        if not flags & 2:
            r.update(chunks=np.zeros((nc_room, 3), np.uint32), cmap=np.zeros(nc_room, np.uint64), cstate=np.zeros(nc_room, np.uint32),
                     base=np.zeros(15 * nc_room + 1, np.uint32), sb=np.zeros(15 * nt + 1, np.uint32),
                     sbits=np.zeros(n // 32 + 16, np.uint32), smap=np.zeros((nsc, 2), np.uint32),
                     snaps=np.zeros(((n + 31) // 32, 2), np.uint32), sstart=np.zeros(nsc, np.uint16))
        o = ModelsOut()
        for k, a in r.items():
            setattr(o, k, _ptr(a))
        if letter == "B":
            _check(self.lib.bwtc_hip_test_models(self.handle, _ptr(packed), n, _ptr(tasks), nt, state_in, flags, ctypes.byref(o)),
                   "bwtc_hip_test_models")
        else:
            _check(self.lib.bwtc_hip_test_models_letter(self.handle, letter.encode(), _ptr(packed), n, _ptr(tasks), nt, state_in, flags,
                                                        ctypes.byref(o)), "bwtc_hip_test_models_letter")
        nc = int(o.nc)
        for k in ("chunks", "cmap", "cstate"):
            if k in r:
                r[k] = r[k][:nc]
        if "base" in r:
            r["base"] = r["base"][:15 * nc + 1]
        r.update(tail=np.array(list(o.tail), np.uint32), ends=np.array(list(o.ends), np.uint32), nc=nc, nsc=int(o.nsc))
        return r

    def copy_probe(self, nbytes=1 << 30, reps=5):
        """GB/s (read + written) of the library's own 16-byte-per-lane copy kernel on this GPU (bwtc_hip_copy_probe)."""
        g = ctypes.c_double(0.0)
        _check(self.lib.bwtc_hip_copy_probe(self.handle, nbytes, reps, ctypes.byref(g)), "bwtc_hip_copy_probe")
        return float(g.value)

    # ---- device buffers without a HIP binding of one's own ------------------------------
    def dmalloc(self, nbytes):
        p = self.lib.bwtc_hip_malloc(self.handle, nbytes)
        if not p:
            raise BwtcHipError("bwtc_hip_malloc(%d) failed" % nbytes)
        return p

    def dfree(self, ptr):
        self.lib.bwtc_hip_free(self.handle, _vp(ptr))

    def to_device(self, d_ptr, arr):
        arr = np.ascontiguousarray(arr)
        _check(self.lib.bwtc_hip_memcpy_to_device(self.handle, _vp(d_ptr), _ptr(arr), arr.nbytes),
               "bwtc_hip_memcpy_to_device")

    def host_alloc(self, nbytes):
        """Page-locked host bytes as a numpy array (freed with host_free, or with the process)."""
        p = self.lib.bwtc_hip_host_alloc(self.handle, nbytes)
        if not p:
            raise BwtcHipError("bwtc_hip_host_alloc(%d) failed" % nbytes)
        arr = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,))
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p
        return arr

    def host_free(self, arr):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p:
            self.lib.bwtc_hip_host_free(self.handle, _vp(p))

    def to_device_async(self, d_ptr, arr):
        """Upload on the context's copy stream; returns at once (arr must stay alive and unchanged
        until copy_wait())."""
        _check(self.lib.bwtc_hip_memcpy_to_device_async(self.handle, _vp(d_ptr), _ptr(arr), arr.nbytes),
               "bwtc_hip_memcpy_to_device_async")

    def copy_wait(self):
        _check(self.lib.bwtc_hip_copy_wait(self.handle), "bwtc_hip_copy_wait")

    def wavelet_host_clock(self):
        """(seconds in the adaptive models, seconds in the range coders, blocks) of the 'B' coder's
        worker threads, summed over threads since the context was made."""
        m, c, b = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_uint64(0)
        _check(self.lib.bwtc_hip_wavelet_host_clock(self.handle, ctypes.byref(m), ctypes.byref(c), ctypes.byref(b)),
               "bwtc_hip_wavelet_host_clock")
        return m.value, c.value, b.value

    def wavelet_set_depth(self, depth):
        """Blocks that may be under way from now on; staging buffers beyond that go back to the system."""
        _check(self.lib.bwtc_hip_wavelet_set_depth(self.handle, int(depth)), "bwtc_hip_wavelet_set_depth")

    def wavelet_depth_needed(self):
        """Blocks to keep under way for the rate shown so far (0 until four blocks have finished)."""
        return int(self.lib.bwtc_hip_wavelet_depth_needed(self.handle))

    def wavelet_latency(self):
        """Mean seconds a block has been under way (device half started -> record finished)."""
        v = ctypes.c_double(0)
        _check(self.lib.bwtc_hip_wavelet_latency(self.handle, ctypes.byref(v)), "bwtc_hip_wavelet_latency")
        return v.value

    def wavelet_routes(self, reset=False):
        """The routes this context's wavelet blocks took so far, one count per block (bwtc_hip.h):
        dict of trees_device, trees_host, models_device, models_rejected, reject_reasons (REJECT_* bits),
        lost_turn, models_host_two_stage, models_host_fused, models_host_lanes.  reset: start again from zero."""
        r = WaveletRouteCounts()
        _check(self.lib.bwtc_hip_wavelet_routes(self.handle, ctypes.byref(r), 1 if reset else 0), "bwtc_hip_wavelet_routes")
        return {f: int(getattr(r, f)) for f, _ in WaveletRouteCounts._fields_}

    def numa_node(self):
        """NUMA node of the context's GPU, -1 when the system does not say."""
        return int(self.lib.bwtc_hip_numa_node(self.handle))

    def set_worker_cpus(self, cpus):
        """The context's worker threads may run on exactly these CPUs (empty: no restriction)."""
        a = np.ascontiguousarray(cpus, np.uint32)
        _check(self.lib.bwtc_hip_set_worker_cpus(self.handle, _ptr(a) if a.size else None, a.size), "bwtc_hip_set_worker_cpus")

    def wavelet_host_progress(self):
        """(blocks that joined the host half, blocks whose record the workers have finished)."""
        q, f = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(self.lib.bwtc_hip_wavelet_host_progress(self.handle, ctypes.byref(q), ctypes.byref(f)),
               "bwtc_hip_wavelet_host_progress")
        return q.value, f.value

    def to_host(self, d_ptr, nbytes):
        out = np.empty(nbytes, np.uint8)
        _check(self.lib.bwtc_hip_memcpy_to_host(self.handle, _ptr(out), _vp(d_ptr), nbytes),
               "bwtc_hip_memcpy_to_host")
        return out

    def bwt_block(self, data, starting_points=8):
        """BWTManager::doTransform(block, freqs): returns (bwt bytes, LFpowers, freqs).

        The buffer handed to the library carries one extra byte after the block, as the
        reference's PrecompressorBlock does, and that byte is checked to be untouched."""
        data = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8)
                                    if not isinstance(data, np.ndarray) else data, dtype=np.uint8)
        size = data.size
        buf = np.empty(size + 1, np.uint8)
        buf[:size] = data
        buf[size] = 0xA5
        n_lf = self.n_lf(size, starting_points)
        lf = np.zeros(n_lf, np.uint32)
        freqs = np.zeros(256, np.uint32)
        _check(self.lib.bwtc_hip_bwt_block(self.handle, _ptr(buf), size, _ptr(lf), n_lf,
                                           _ptr(freqs)), "bwtc_hip_bwt_block")
        if buf[size] != 0xA5:
            raise BwtcHipError("byte after the block was modified")
        return buf[:size].copy(), lf, freqs

    def bwt_raw(self, T, n_lf=1, freqs=None):
        """BWTransform::doTransform(begin, length, LF, freqs) on T (sentinel included)."""
        T = np.array(T, dtype=np.uint8, copy=True)
        lf = np.zeros(n_lf, np.uint32)
        fr = np.zeros(256, np.uint32) if freqs is None else freqs
        _check(self.lib.bwtc_hip_bwt(self.handle, _ptr(T), T.size, _ptr(lf), n_lf, _ptr(fr)),
               "bwtc_hip_bwt")
        return T, lf, fr

    def bwt_block_device(self, d_in_ptr, d_out_ptr, size, starting_points=8):
        n_lf = self.n_lf(size, starting_points)
        lf = np.zeros(n_lf, np.uint32)
        freqs = np.zeros(256, np.uint32)
        _check(self.lib.bwtc_hip_bwt_block_device(self.handle, _vp(d_in_ptr), _vp(d_out_ptr), size,
                                                  _ptr(lf), n_lf, _ptr(freqs)),
               "bwtc_hip_bwt_block_device")
        return lf, freqs

    def _batch_items(self, offsets, sizes, starting_points):
        items = (BatchItem * len(sizes))()
        for i, (off, size) in enumerate(zip(offsets, sizes)):
            items[i].offset, items[i].size = int(off), int(size)
            items[i].n_lf = self.n_lf(int(size), starting_points) if size else 1
        return items

    def bwt_blocks(self, blocks, starting_points=8):
        """bwtc_hip_bwt_blocks: every block of the list in one batched call; a list of (bwt bytes, LFpowers,
        freqs), each as bwt_block gives it.  The blocks lie side by side in one buffer with a guard byte after each,
        which is checked to be untouched."""
        arrs = [np.ascontiguousarray(np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else b,
                                     dtype=np.uint8) for b in blocks]
        sizes = [a.size for a in arrs]
        offsets = [0] * len(arrs)
        for i in range(1, len(arrs)):
            offsets[i] = offsets[i - 1] + sizes[i - 1] + 1
        buf = np.full(sum(sizes) + len(sizes) + 1, 0xA5, np.uint8)
        for a, off in zip(arrs, offsets):
            buf[off:off + a.size] = a
        items = self._batch_items(offsets, sizes, starting_points)
        lf = np.zeros((max(len(arrs), 1), 256), np.uint32)
        freqs = np.zeros((max(len(arrs), 1), 256), np.uint32)
        _check(self.lib.bwtc_hip_bwt_blocks(self.handle, _ptr(buf), ctypes.cast(items, _vp), len(arrs), _ptr(lf), _ptr(freqs)),
               "bwtc_hip_bwt_blocks")
        for off, size in zip(offsets, sizes):
            if buf[off + size] != 0xA5:
                raise BwtcHipError("byte after a block was modified")
        return [(buf[off:off + size].copy(), lf[i, :items[i].n_lf].copy(), freqs[i].copy())
                for i, (off, size) in enumerate(zip(offsets, sizes))]

    def bwt_blocks_device(self, d_in_ptr, d_out_ptr, offsets, sizes, starting_points=8, n_lf=None):
        """bwtc_hip_bwt_blocks_device over device pointers (they may be the same): block i is `sizes[i]` bytes at
        `offsets[i]` of both.  Returns (lf rows [k, 256], freqs rows [k, 256], the n_lf of every block); n_lf: the
        blocks' numbers of LF powers where they are not to come from n_lf()."""
        items = self._batch_items(offsets, sizes, starting_points)
        if n_lf is not None:
            for i, v in enumerate(n_lf):
                items[i].n_lf = int(v)
        k = len(sizes)
        lf = np.zeros((max(k, 1), 256), np.uint32)
        freqs = np.zeros((max(k, 1), 256), np.uint32)
        _check(self.lib.bwtc_hip_bwt_blocks_device(self.handle, _vp(d_in_ptr), _vp(d_out_ptr), ctypes.cast(items, _vp), k,
                                                   _ptr(lf), _ptr(freqs)), "bwtc_hip_bwt_blocks_device")
        return lf, freqs, [int(items[i].n_lf) for i in range(k)]

    def batch_stats(self):
        """bwtc_hip_batch_stats_get as a dict (active: the entries left after the initial sort and after every round)."""
        s = BatchStats()
        _check(self.lib.bwtc_hip_batch_stats_get(self.handle, ctypes.byref(s)), "bwtc_hip_batch_stats_get")
        d = {f: getattr(s, f) for f in ("blocks", "stride_log2", "rounds", "host_waits", "suffixes", "ms_total")}
        d["active"] = [int(v) for v in s.active][:min(int(s.rounds), 31) + 1]
        return d

    def test_batch_keys(self, data, offsets, sizes):
        """bwtc_hip_test_batch_keys: the load pass and the initial keys of the blocks at `offsets` of `data`:
        (T of every block one after the other, keys in the same order, counts [k, 256])."""
        data = np.ascontiguousarray(data, np.uint8)
        items = self._batch_items(offsets, sizes, 1)
        m = int(sum(sizes)) + len(sizes)
        T = np.zeros(m, np.uint8)
        keys = np.zeros(m, np.uint64)
        freqs = np.zeros((max(len(sizes), 1), 256), np.uint32)
        _check(self.lib.bwtc_hip_test_batch_keys(self.handle, _ptr(data), ctypes.cast(items, _vp), len(sizes), _ptr(T), _ptr(keys),
                                                 _ptr(freqs)), "bwtc_hip_test_batch_keys")
        return T, keys, freqs

    def inverse_bwt_block(self, bwt, lf):
        """InverseBWTransform::doTransform(BWTBlock&): returns the original block; raises
        BwtcHipError (code -4) when an LF power does not lie on the LF walk."""
        b = np.array(bwt, dtype=np.uint8, copy=True)
        lf = np.ascontiguousarray(lf, dtype=np.uint32)
        _check(self.lib.bwtc_hip_inverse_bwt_block(self.handle, _ptr(b), b.size, _ptr(lf), lf.size),
               "bwtc_hip_inverse_bwt_block")
        return b

    def inverse_bwt_block_device(self, d_bwt_ptr, d_out_ptr, size, lf):
        lf = np.ascontiguousarray(lf, dtype=np.uint32)
        _check(self.lib.bwtc_hip_inverse_bwt_block_device(self.handle, _vp(d_bwt_ptr), _vp(d_out_ptr),
                                                          size, _ptr(lf), lf.size),
               "bwtc_hip_inverse_bwt_block_device")

    def wavelet_section_stats(self, bwt, freqs):
        """utils::calculateRunsAndCharacters per section (WaveletTree ctor front-end): returns
        (section lengths, run_freqs[section][256], total runs, [dict(length -> count)])."""
        bwt = np.ascontiguousarray(bwt, dtype=np.uint8)
        freqs = np.ascontiguousarray(freqs, dtype=np.uint32)
        nsec = _u32(0)
        sec = np.zeros(256, np.uint32)
        rf = np.zeros(256 * 256, np.uint32)
        tot = np.zeros(256, np.uint64)
        off = np.zeros(257, np.uint32)
        cap = max(1 << 16, bwt.size // 8 + 4096)
        dl = np.zeros(cap, np.uint32)
        dc = np.zeros(cap, np.uint32)
        _check(self.lib.bwtc_hip_wavelet_section_stats(self.handle, _ptr(bwt), bwt.size, _ptr(freqs),
                                                       ctypes.byref(nsec), _ptr(sec), _ptr(rf), _ptr(tot),
                                                       _ptr(off), _ptr(dl), _ptr(dc), cap),
               "bwtc_hip_wavelet_section_stats")
        n = nsec.value
        dist = [dict(zip(dl[off[s]:off[s + 1]].tolist(), dc[off[s]:off[s + 1]].tolist())) for s in range(n)]
        return sec[:n].copy(), rf.reshape(256, 256)[:n].copy(), tot[:n].copy(), dist

    def wavelet_reset(self):
        """Start a new stream: the 'B' coder's carried model state goes back to its initial value."""
        self.lib.bwtc_hip_wavelet_reset(self.handle)

    def wavelet_encode(self, bwt, lf, freqs, threads=0):
        """WaveletEncoder ('B'): writeBlockHeader + encodeData + finishBlock on a transformed block."""
        bwt = np.ascontiguousarray(bwt, dtype=np.uint8)
        lf = np.ascontiguousarray(lf, dtype=np.uint32)
        freqs = np.ascontiguousarray(freqs, dtype=np.uint32)
        cap = self.compress_bound(bwt.size)
        out = np.zeros(cap, np.uint8)
        n = _u64(0)
        _check(self.lib.bwtc_hip_wavelet_encode(self.handle, _ptr(bwt), bwt.size, _ptr(lf), lf.size,
                                                _ptr(freqs), threads, _ptr(out), cap, ctypes.byref(n)),
               "bwtc_hip_wavelet_encode")
        return out[:n.value].copy()

    def wavelet_encode_device(self, d_bwt_ptr, size, lf, freqs, out, threads=0):
        """Same on a device-resident block; `out` is a host uint8 array; returns bytes written."""
        lf = np.ascontiguousarray(lf, dtype=np.uint32)
        freqs = np.ascontiguousarray(freqs, dtype=np.uint32)
        n = _u64(0)
        _check(self.lib.bwtc_hip_wavelet_encode_device(self.handle, _vp(d_bwt_ptr), size, _ptr(lf), lf.size,
                                                       _ptr(freqs), threads, _ptr(out), out.size,
                                                       ctypes.byref(n)),
               "bwtc_hip_wavelet_encode_device")
        return int(n.value)

    def wavelet_start(self, coder="B"):
        """New wavelet stream with the main model of coder letter `coder` ('B', 'b' or 'u')."""
        _check(self.lib.bwtc_hip_wavelet_start(self.handle, coder.encode()), "bwtc_hip_wavelet_start")

    def wavelet_encode_device_begin(self, d_bwt_ptr, size, lf, freqs, out, threads=0):
        """First half: device work now, models + range coder queued on the worker threads.
        `out` must stay alive until wavelet_encode_end(ticket); returns the ticket."""
        lf = np.ascontiguousarray(lf, dtype=np.uint32)
        freqs = np.ascontiguousarray(freqs, dtype=np.uint32)
        t = _u64(0)
        _check(self.lib.bwtc_hip_wavelet_encode_device_begin(self.handle, _vp(d_bwt_ptr), size, _ptr(lf), lf.size,
                                                             _ptr(freqs), threads, _ptr(out), out.size,
                                                             ctypes.byref(t)),
               "bwtc_hip_wavelet_encode_device_begin")
        return int(t.value)

    def wavelet_encode_device_prepare(self, d_bwt_ptr, size, lf, freqs, out, threads=0):
        """The half of _begin that needs nothing from earlier blocks (all the device work)."""
        lf = np.ascontiguousarray(lf, dtype=np.uint32)
        freqs = np.ascontiguousarray(freqs, dtype=np.uint32)
        t = _u64(0)
        _check(self.lib.bwtc_hip_wavelet_encode_device_prepare(self.handle, _vp(d_bwt_ptr), size, _ptr(lf), lf.size,
                                                               _ptr(freqs), threads, _ptr(out), out.size,
                                                               ctypes.byref(t)),
               "bwtc_hip_wavelet_encode_device_prepare")
        return int(t.value)

    def wavelet_encode_queue(self, ticket, state_in):
        """Gives a prepared block its place in a stream; returns the carried state after it."""
        st = _u32(0)
        _check(self.lib.bwtc_hip_wavelet_encode_queue(self.handle, ticket, state_in, ctypes.byref(st)),
               "bwtc_hip_wavelet_encode_queue")
        return int(st.value)

    def wavelet_encode_end(self, ticket):
        """Second half: waits for the block, returns the record's size."""
        n = _u64(0)
        _check(self.lib.bwtc_hip_wavelet_encode_end(self.handle, _u64(ticket), ctypes.byref(n)),
               "bwtc_hip_wavelet_encode_end")
        return int(n.value)

    def transform_and_encode_wavelet(self, data, starting_points=8, threads=0):
        """WaveletEncoder::transformAndEncode ('B'): returns (record, bwt bytes)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        buf = np.empty(data.size + 1, np.uint8)
        buf[:data.size] = data
        buf[data.size] = 0x5A
        cap = self.compress_bound(data.size)
        out = np.zeros(cap, np.uint8)
        n = _u64(0)
        _check(self.lib.bwtc_hip_transform_and_encode_wavelet(self.handle, _ptr(buf), data.size,
                                                              starting_points, threads, _ptr(out), cap,
                                                              ctypes.byref(n)),
               "bwtc_hip_transform_and_encode_wavelet")
        if buf[data.size] != 0x5A:
            raise BwtcHipError("byte after the block was modified")
        return out[:n.value].copy(), buf[:data.size].copy()

    def compress_bound(self, size):
        return int(self.lib.bwtc_hip_compress_bound(size))

    def huffman_encode_device(self, d_bwt_ptr, size, lf, freqs, d_out_ptr, out_cap=None):
        """HuffmanEncoder: writeBlockHeader + encodeData + finishBlock on a device-resident
        transformed block; returns the number of bytes written at d_out_ptr."""
        lf = np.ascontiguousarray(lf, dtype=np.uint32)
        freqs = np.ascontiguousarray(freqs, dtype=np.uint32)
        n = _u64(0)
        cap = self.compress_bound(size) if out_cap is None else out_cap
        _check(self.lib.bwtc_hip_huffman_encode_device(self.handle, _vp(d_bwt_ptr), size, _ptr(lf),
                                                       lf.size, _ptr(freqs), _vp(d_out_ptr), cap,
                                                       ctypes.byref(n)),
               "bwtc_hip_huffman_encode_device")
        return int(n.value)

    def huffman_encode(self, bwt, lf, freqs):
        bwt = np.ascontiguousarray(bwt, dtype=np.uint8)
        lf = np.ascontiguousarray(lf, dtype=np.uint32)
        freqs = np.ascontiguousarray(freqs, dtype=np.uint32)
        cap = self.compress_bound(bwt.size)
        out = np.zeros(cap, np.uint8)
        n = _u64(0)
        _check(self.lib.bwtc_hip_huffman_encode(self.handle, _ptr(bwt), bwt.size, _ptr(lf), lf.size,
                                                _ptr(freqs), _ptr(out), cap, ctypes.byref(n)),
               "bwtc_hip_huffman_encode")
        return out[:n.value].copy()

    def transform_and_encode(self, data, starting_points=8):
        """HuffmanEncoder::transformAndEncode: returns (encoded BWT-block record, bwt bytes)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        buf = np.empty(data.size + 1, np.uint8)
        buf[:data.size] = data
        buf[data.size] = 0x5A
        cap = self.compress_bound(data.size)
        out = np.zeros(cap, np.uint8)
        n = _u64(0)
        _check(self.lib.bwtc_hip_transform_and_encode(self.handle, _ptr(buf), data.size,
                                                      starting_points, _ptr(out), cap,
                                                      ctypes.byref(n)),
               "bwtc_hip_transform_and_encode")
        if buf[data.size] != 0x5A:
            raise BwtcHipError("byte after the block was modified")
        return out[:n.value].copy(), buf[:data.size].copy()

    def huffman_decode(self, record, cap=None):
        """HuffmanDecoder::decodeBlock on the GPU: an 'H' BWT-block record (it may go on past the
        record) -> (bwt bytes, LF powers, bytes of the record consumed)."""
        record = np.ascontiguousarray(record, dtype=np.uint8)
        cap = self.max_block_size if cap is None else cap
        bwt = np.empty(max(cap, 1), np.uint8)
        lf = np.zeros(256, np.uint32)
        n_lf, size, used = _u32(0), _u32(0), _u64(0)
        _check(self.lib.bwtc_hip_huffman_decode(self.handle, _ptr(record), record.size, _ptr(bwt), cap, _ptr(lf),
                                                ctypes.byref(n_lf), ctypes.byref(size), ctypes.byref(used)),
               "bwtc_hip_huffman_decode")
        return bwt[:size.value].copy(), lf[:n_lf.value].copy(), int(used.value)

    def huffman_decode_device(self, d_rec_ptr, rec_bytes, d_bwt_ptr, cap):
        """Same with the record and the bwt bytes in device memory: returns (size, LF powers, consumed)."""
        lf = np.zeros(256, np.uint32)
        n_lf, size, used = _u32(0), _u32(0), _u64(0)
        _check(self.lib.bwtc_hip_huffman_decode_device(self.handle, _vp(d_rec_ptr), rec_bytes, _vp(d_bwt_ptr), cap,
                                                       _ptr(lf), ctypes.byref(n_lf), ctypes.byref(size),
                                                       ctypes.byref(used)),
               "bwtc_hip_huffman_decode_device")
        return int(size.value), lf[:n_lf.value].copy(), int(used.value)

    def decode_block_H(self, record, cap=None, with_consumed=False):
        """Entropy decode + inverse BWT of one 'H' record on the GPU: returns the original block
        (and the bytes consumed when with_consumed)."""
        record = np.ascontiguousarray(record, dtype=np.uint8)
        cap = self.max_block_size if cap is None else cap
        out = np.empty(max(cap, 1), np.uint8)
        size, used = _u32(0), _u64(0)
        _check(self.lib.bwtc_hip_decode_block_H(self.handle, _ptr(record), record.size, _ptr(out), cap,
                                                ctypes.byref(size), ctypes.byref(used)),
               "bwtc_hip_decode_block_H")
        data = out[:size.value].copy()
        return (data, int(used.value)) if with_consumed else data

    def decode_block_H_device(self, record, d_out_ptr, cap):
        """decode_block_H with the original block left in device memory at d_out_ptr: returns (size, consumed)."""
        record = np.ascontiguousarray(record, dtype=np.uint8)
        size, used = _u32(0), _u64(0)
        _check(self.lib.bwtc_hip_decode_block_H_device(self.handle, _ptr(record), record.size, _vp(d_out_ptr), cap,
                                                       ctypes.byref(size), ctypes.byref(used)),
               "bwtc_hip_decode_block_H_device")
        return int(size.value), int(used.value)

    def huffman_decode_stats(self):
        s = HuffmanDecodeStats()
        _check(self.lib.bwtc_hip_huffman_decode_stats_get(self.handle, ctypes.byref(s)),
               "bwtc_hip_huffman_decode_stats_get")
        return {f: getattr(s, f) for f, _ in HuffmanDecodeStats._fields_}

    def decode_block_W(self, decoder, record, cap=None, with_consumed=False):
        """Range decode (host) + wavelet rebuild + inverse BWT (device) of one 'B' / 'b' / 'u' record: returns the
        original block (and the bytes consumed when with_consumed).  decoder: the stream's WaveletDecoder."""
        record = np.ascontiguousarray(record, dtype=np.uint8)
        cap = self.max_block_size if cap is None else cap
        out = np.empty(max(cap, 1), np.uint8)
        size, used = _u32(0), _u64(0)
        _check(self.lib.bwtc_hip_decode_block_W(self.handle, decoder.h, _ptr(record), record.size, _ptr(out), cap,
                                                ctypes.byref(size), ctypes.byref(used)),
               "bwtc_hip_decode_block_W")
        data = out[:size.value].copy()
        return (data, int(used.value)) if with_consumed else data

    def decode_block_W_device(self, decoder, record, d_out_ptr, cap):
        """decode_block_W with the original block left in device memory at d_out_ptr: returns (size, consumed)."""
        record = np.ascontiguousarray(record, dtype=np.uint8)
        size, used = _u32(0), _u64(0)
        _check(self.lib.bwtc_hip_decode_block_W_device(self.handle, decoder.h, _ptr(record), record.size, _vp(d_out_ptr), cap,
                                                       ctypes.byref(size), ctypes.byref(used)),
               "bwtc_hip_decode_block_W_device")
        return int(size.value), int(used.value)

    def decode_block_W_begin(self, decoder, record, cap, slot):
        """The host half of decode_block_W into forest slot `slot` (0 / 1): returns (block bytes, consumed)."""
        record = np.ascontiguousarray(record, dtype=np.uint8)
        size, used = _u32(0), _u64(0)
        _check(self.lib.bwtc_hip_decode_block_W_begin(self.handle, decoder.h, _ptr(record), record.size, cap, slot,
                                                      ctypes.byref(size), ctypes.byref(used)),
               "bwtc_hip_decode_block_W_begin")
        return int(size.value), int(used.value)

    def decode_block_W_end(self, slot, cap):
        """The device half of slot `slot`: the original block."""
        out = np.empty(max(cap, 1), np.uint8)
        size = _u32(0)
        _check(self.lib.bwtc_hip_decode_block_W_end(self.handle, slot, _ptr(out), cap, ctypes.byref(size)),
               "bwtc_hip_decode_block_W_end")
        return out[:size.value].copy()

    def decode_block_W_end_device(self, slot, d_out_ptr, cap):
        size = _u32(0)
        _check(self.lib.bwtc_hip_decode_block_W_end_device(self.handle, slot, _vp(d_out_ptr), cap, ctypes.byref(size)),
               "bwtc_hip_decode_block_W_end_device")
        return int(size.value)

    def wavelet_rebuild(self, forest, cap=None):
        """Flattened forest (Forest) -> BWT bytes through the device kernels, host to host."""
        cap = forest.total if cap is None else cap
        out = np.full(cap + 64, 0xA5, np.uint8)
        size = _u64(0)
        _check(self.lib.bwtc_hip_wavelet_rebuild(self.handle, ctypes.byref(forest.c), _ptr(out), cap, ctypes.byref(size)),
               "bwtc_hip_wavelet_rebuild")
        return out[:size.value].copy()

    def wavelet_rebuild_device(self, forest, d_out_ptr, cap):
        """Same with the bytes left in device memory at d_out_ptr (any alignment): returns their number."""
        size = _u64(0)
        _check(self.lib.bwtc_hip_wavelet_rebuild_device(self.handle, ctypes.byref(forest.c), _vp(d_out_ptr), cap, ctypes.byref(size)),
               "bwtc_hip_wavelet_rebuild_device")
        return int(size.value)

    def wavelet_decode_stats(self):
        s = WaveletDecodeStats()
        _check(self.lib.bwtc_hip_wavelet_decode_stats_get(self.handle, ctypes.byref(s)),
               "bwtc_hip_wavelet_decode_stats_get")
        return {f: getattr(s, f) for f, _ in WaveletDecodeStats._fields_}

    def suffix_array(self, T):
        T = np.ascontiguousarray(T, dtype=np.uint8)
        sa = np.zeros(T.size, np.uint32)
        _check(self.lib.bwtc_hip_suffix_array(self.handle, _ptr(T), T.size, _ptr(sa)),
               "bwtc_hip_suffix_array")
        return sa

    def test_sort(self, keys, vals, nbits):
        keys = np.array(keys, copy=True)
        vals = np.array(vals, dtype=np.uint32, copy=True)
        fn = self.lib.bwtc_hip_test_sort_u64 if keys.dtype == np.uint64 else self.lib.bwtc_hip_test_sort_u32
        _check(fn(self.handle, _ptr(keys), _ptr(vals), keys.size, nbits), "bwtc_hip_test_sort")
        return keys, vals

    def test_scan(self, data):
        data = np.array(data, dtype=np.uint32, copy=True)
        _check(self.lib.bwtc_hip_test_scan_u32(self.handle, _ptr(data), data.size), "bwtc_hip_test_scan")
        return data

    # radix_sort.hpp's three sorts, called directly (bwtc_hip_test_radix_*): a contract the hook refuses raises
    # BwtcHipError with code -1, a changed canary behind a buffer with code -20 - its index
    RADIX_VALUES = {"given": 0, "positions": 1, "keys": 2, "descending": 3}

    def test_radix_pairs(self, keys, vals=None, n_holes=0, bit_lo=0, nbits=None, values="given", planes=0, vtype=np.uint32):
        """keys (uint32 | uint64): n + n_holes slots, of which n_holes all ones.  -> (n sorted keys, their values or None).
        values: "given" (vals, one per slot), "positions", "descending" or "keys"; planes 0 off, 1 on, 2 on with the first
        pass's plane ready (made by the hook); vtype uint32 | uint16."""
        keys = np.array(keys, copy=True)
        assert keys.dtype in (np.uint32, np.uint64) and keys.ndim == 1
        vtype = np.dtype(vtype)
        n = keys.size - n_holes
        mode = self.RADIX_VALUES[values]
        if mode == 0:
            vals = np.array(vals, dtype=vtype, copy=True)
            assert vals.size == keys.size
        elif mode != 2:
            vals = np.zeros(max(n, 1), vtype)
        else:
            vals = None
        nbits = 8 * keys.itemsize if nbits is None else nbits
        _check(self.lib.bwtc_hip_test_radix_pairs(self.handle, _ptr(keys), None if vals is None else _ptr(vals), n, n_holes, keys.itemsize,
                                                  vtype.itemsize, bit_lo, nbits, mode, planes), "bwtc_hip_test_radix_pairs")
        return keys[:n], (None if vals is None else vals[:n])

    def test_radix_long(self, keys, w, kbits, wbits, vtype=np.uint32, items_per_thread=6, direct_w=True):
        """Long items (uint64 keys, uint32 w) -> (keys, values, w) sorted by (keys bits [0, kbits), w bits [0, wbits));
        the values are n - 1 - (first place), cut to vtype."""
        keys = np.array(keys, dtype=np.uint64, copy=True)
        w = np.array(w, dtype=np.uint32, copy=True)
        assert keys.size == w.size
        vals = np.zeros(max(keys.size, 1), np.dtype(vtype))
        _check(self.lib.bwtc_hip_test_radix_long(self.handle, _ptr(keys), _ptr(vals), _ptr(w), keys.size, vals.itemsize, items_per_thread,
                                                 kbits, wbits, 1 if direct_w else 0), "bwtc_hip_test_radix_long")
        return keys, vals[:keys.size], w

    def test_radix_segmented(self, keys, bit_lo, tile_first):
        """uint32 keys in whole tiles of 8192, segment s = tiles [tile_first[s], tile_first[s + 1]) -> every segment
        sorted on its own by bits [bit_lo, bit_lo + 16)."""
        keys = np.array(keys, dtype=np.uint32, copy=True)
        tf = np.array(tile_first, dtype=np.uint32, copy=True)
        assert tf.size >= 2
        _check(self.lib.bwtc_hip_test_radix_segmented(self.handle, _ptr(keys), keys.size, bit_lo, _ptr(tf), tf.size - 1),
               "bwtc_hip_test_radix_segmented")
        return keys

    # the suffix sorter's period step
    def period(self):
        """The last block's (period, longest periodic stretch, the winner's votes, depth of the period step): zeros
        where nothing was looked for, nothing was found or no step ran (bwtc_hip_period_get)."""
        v = [_u32(0) for _ in range(4)]
        _check(self.lib.bwtc_hip_period_get(self.handle, *[ctypes.byref(x) for x in v]), "bwtc_hip_period_get")
        return tuple(int(x.value) for x in v)

    def steps(self):
        """The last block's closed-form steps (bwtc_hip_steps_get): (depth of the run step, the period step's period, its
        depth, the longest run, the longest proper stretch); depths 0 for a step that did not run."""
        v = [_u32(0) for _ in range(5)]
        _check(self.lib.bwtc_hip_steps_get(self.handle, *[ctypes.byref(x) for x in v]), "bwtc_hip_steps_get")
        return tuple(int(x.value) for x in v)

    def test_period_proper(self, T, p, k_out=None):
        """test_period_lengths() by the pass with the second maximum (bwtc_hip_test_period_proper) -> (k_p[], the longest,
        the longest proper stretch)."""
        T = np.ascontiguousarray(T, dtype=np.uint8)
        if k_out is None:
            k_out = np.zeros(max(T.size, 1), np.uint32)
        assert k_out.dtype == np.uint32 and k_out.size >= T.size
        longest, proper = _u32(0), _u32(0)
        _check(self.lib.bwtc_hip_test_period_proper(self.handle, _ptr(T) if T.size else None, T.size, int(p), _ptr(k_out),
                                                    ctypes.byref(longest), ctypes.byref(proper)), "bwtc_hip_test_period_proper")
        return k_out[:T.size], int(longest.value), int(proper.value)

    def schedule(self):
        """The last block's schedule of closed-form steps (bwtc_hip_schedule_get), in the order it took them:
        [(period, depth it ran at or 0, gate length, votes, flags)], flags 1: ranked the runs too, 2: dropped."""
        w, found = np.zeros(5 * 8, np.uint32), _u32(0)
        _check(self.lib.bwtc_hip_schedule_get(self.handle, _ptr(w), 8, ctypes.byref(found)), "bwtc_hip_schedule_get")
        return [tuple(int(x) for x in w[5 * i:5 * i + 5]) for i in range(min(int(found.value), 8))]

    # the suffix sorter's copy rounds (BWTC_HIP_COPIES=1)
    def copies(self):
        """The last block's copy rounds (bwtc_hip_copies_get): (rounds that looked up at K[s] + h, passes that made K[], the
        longest K, the depth of the first copy round); zeros without the switch or where no round took a pass."""
        v = [_u32(0) for _ in range(4)]
        _check(self.lib.bwtc_hip_copies_get(self.handle, *[ctypes.byref(x) for x in v]), "bwtc_hip_copies_get")
        return tuple(int(x.value) for x in v)

    def test_copy_lengths(self, suf, grp, rank, k_out=None):
        """The copy round's three passes over a list (suffix and dense group number per entry, in list order) and rank[]
        (bwtc_hip_test_copy_lengths) -> (K[], the longest).  A contract the hook refuses raises BwtcHipError with code -1
        (k_out is left untouched), a changed canary with code -20 - its index."""
        suf = np.ascontiguousarray(suf, dtype=np.uint32)
        grp = np.ascontiguousarray(grp, dtype=np.uint32)
        rank = np.ascontiguousarray(rank, dtype=np.uint32)
        assert suf.size == grp.size
        if k_out is None:
            k_out = np.zeros(max(rank.size, 1), np.uint32)
        assert k_out.dtype == np.uint32 and k_out.size >= rank.size
        longest = _u32(0)
        _check(self.lib.bwtc_hip_test_copy_lengths(self.handle, _ptr(suf) if suf.size else None, _ptr(grp) if grp.size else None, suf.size,
                                                   _ptr(rank) if rank.size else None, rank.size, _ptr(k_out), ctypes.byref(longest)),
               "bwtc_hip_test_copy_lengths")
        return k_out[:rank.size], int(longest.value)

    def test_period_merge(self, T, p, h, k=None):
        """The merging storing pass of BWTC_HIP_MULTI (bwtc_hip_test_period_merge) for the step of period p at depth h.  k:
        the uint32 array of the block's merged words, read and written in place; None: the block's first step (fresh).
        -> (the words, the longest stretch, the longest proper stretch)."""
        T = np.ascontiguousarray(T, dtype=np.uint8)
        fresh = k is None
        if fresh:
            k = np.zeros(max(T.size, 1), np.uint32)
        assert k.dtype == np.uint32 and k.size >= T.size and k.flags.c_contiguous
        longest, proper = _u32(0), _u32(0)
        _check(self.lib.bwtc_hip_test_period_merge(self.handle, _ptr(T) if T.size else None, T.size, int(p), int(h), 1 if fresh else 0, _ptr(k),
                                                   ctypes.byref(longest), ctypes.byref(proper)), "bwtc_hip_test_period_merge")
        return k[:T.size], int(longest.value), int(proper.value)

    def test_period_winners(self, table, need):
        """The finder's candidates over a vote table of 4097 words (bwtc_hip_test_period_winners) -> [(distance, votes)],
        at most 8, and the 16 words as the kernel left them."""
        table = np.ascontiguousarray(table, dtype=np.uint32)
        assert table.size == 4097
        out, found = np.full(16, 0xABCD1234, np.uint32), _u32(0)
        _check(self.lib.bwtc_hip_test_period_winners(self.handle, _ptr(table), int(need), _ptr(out), ctypes.byref(found)),
               "bwtc_hip_test_period_winners")
        return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(int(found.value))], out

    def test_period_lengths(self, T, p, k_out=None):
        """The sorter's own period-length pass over T (bwtc_hip_test_period_lengths) -> (k_p[], the longest).  k_out: the
        uint32 array to fill (left untouched where the hook refuses: BwtcHipError, code -1)."""
        T = np.ascontiguousarray(T, dtype=np.uint8)
        if k_out is None:
            k_out = np.zeros(max(T.size, 1), np.uint32)
        assert k_out.dtype == np.uint32 and k_out.size >= T.size
        longest = _u32(0)
        _check(self.lib.bwtc_hip_test_period_lengths(self.handle, _ptr(T) if T.size else None, T.size, int(p), _ptr(k_out), ctypes.byref(longest)),
               "bwtc_hip_test_period_lengths")
        return k_out[:T.size], int(longest.value)

    # the suffix sorter's long periods (BWTC_HIP_LONG_PERIODS=1: periods 4097 ... 2^24)
    def test_long_period_votes(self, ks, vs, kmask, need, k1=None):
        """The long finder's two sweeps and merged candidates over a sorted list (bwtc_hip_test_long_period_votes): ks the
        uint64 keys, vs the uint32 suffixes, k1 the runs' lengths for the rule that two members of one run do not vote.
        -> ([(distance, votes)], at most 8, and 24 words: the 16 the hook wrote and 8 guard words 0xABCD1234 behind them).
        A contract the hook refuses raises BwtcHipError with code -1."""
        ks = np.ascontiguousarray(ks, dtype=np.uint64)
        vs = np.ascontiguousarray(vs, dtype=np.uint32)
        assert ks.size == vs.size
        if k1 is not None:
            k1 = np.ascontiguousarray(k1, dtype=np.uint32)
            assert vs.size == 0 or k1.size > int(vs.max())
        out, found = np.full(24, 0xABCD1234, np.uint32), _u32(0)
        _check(self.lib.bwtc_hip_test_long_period_votes(self.handle, _ptr(ks) if ks.size else None, _ptr(vs) if vs.size else None, ks.size,
                                                        int(kmask), None if k1 is None else _ptr(k1), int(need), _ptr(out), ctypes.byref(found)),
               "bwtc_hip_test_long_period_votes")
        return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(int(found.value))], out

    def test_long_period_probe(self, T, p, span):
        """The wide probe over T (bwtc_hip_test_long_period_probe) -> True when an aligned window of `span` positions,
        p + i * span on, holds no break of period p."""
        T = np.ascontiguousarray(T, dtype=np.uint8)
        flag = _u32(0xABCD1234)
        _check(self.lib.bwtc_hip_test_long_period_probe(self.handle, _ptr(T) if T.size else None, T.size, int(p), int(span), ctypes.byref(flag)),
               "bwtc_hip_test_long_period_probe")
        assert flag.value in (0, 1), flag.value
        return flag.value == 1

    def test_long_period_lengths(self, T, p, k_out=None):
        """The sorter's period-length pass with both maxima for 4097 <= p <= 2^24, p < len(T)
        (bwtc_hip_test_long_period_lengths) -> (k_p[], the longest, the longest proper stretch).  k_out: the uint32 array to
        fill (left untouched where the hook refuses: BwtcHipError, code -1)."""
        T = np.ascontiguousarray(T, dtype=np.uint8)
        if k_out is None:
            k_out = np.zeros(max(T.size, 1), np.uint32)
        assert k_out.dtype == np.uint32 and k_out.size >= T.size
        two = np.zeros(2, np.uint32)
        _check(self.lib.bwtc_hip_test_long_period_lengths(self.handle, _ptr(T) if T.size else None, T.size, int(p), _ptr(k_out), _ptr(two)),
               "bwtc_hip_test_long_period_lengths")
        return k_out[:T.size], int(two[0]), int(two[1])

    # the suffix sorter's code-key stage, kernel by kernel (bwtc_hip_test_code_*): a
    # contract the hook refuses raises BwtcHipError with code -1, a changed canary with code -20 - its index
    def test_code_stage(self, T, lone_sentinel, code_bits=72, split=True, want_keys=True):
        """The whole stage over T as the sorter holds it -> dict(lut, sigma, counts (256 x 256, summed over the replicas),
        table (257 x 256), err, and -- want_keys -- keys, w, plane, slot j for suffix n - 1 - j)."""
        T = np.ascontiguousarray(T, dtype=np.uint8)
        n = T.size
        lut, counts, table = np.zeros(256, np.uint8), np.zeros((256, 256), np.uint32), np.zeros((257, 256), np.uint32)
        sigma, err = _u32(0), _u32(0)
        keys = np.zeros(n, np.uint64) if want_keys else None
        w = np.zeros(n, np.uint32) if want_keys else None
        plane = np.zeros(n, np.uint8) if want_keys else None
        opt = lambda a: _ptr(a) if a is not None and a.size else None
        _check(self.lib.bwtc_hip_test_code_stage(self.handle, opt(T), n, 1 if lone_sentinel else 0, int(code_bits), 1 if split else 0, _ptr(lut),
                                                 ctypes.byref(sigma), _ptr(counts), _ptr(table), ctypes.byref(err), opt(keys), opt(w), opt(plane)),
               "bwtc_hip_test_code_stage")
        return dict(lut=lut, sigma=int(sigma.value), counts=counts, table=table, err=int(err.value), keys=keys, w=w, plane=plane)

    def test_code_table(self, counts, sigma):
        """k_code_build alone over one replica's 256 x 256 counts -> (table (257 x 256), the error word)."""
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        assert counts.size == 65536
        table, err = np.zeros((257, 256), np.uint32), _u32(0)
        _check(self.lib.bwtc_hip_test_code_table(self.handle, _ptr(counts), int(sigma), _ptr(table), ctypes.byref(err)), "bwtc_hip_test_code_table")
        return table, int(err.value)

    def test_code_keys(self, T, lut, sigma, table, code_bits=72, split=True):
        """k_make_keys_code alone with the caller's dense codes and table -> (keys, w, plane)."""
        T = np.ascontiguousarray(T, dtype=np.uint8)
        lut = np.ascontiguousarray(lut, dtype=np.uint8)
        table = np.ascontiguousarray(table, dtype=np.uint32)
        assert lut.size == 256 and table.size == 257 * 256
        n = T.size
        keys, w, plane = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint8)
        _check(self.lib.bwtc_hip_test_code_keys(self.handle, _ptr(T) if n else None, n, int(code_bits), 1 if split else 0, _ptr(lut), int(sigma),
                                                _ptr(table), _ptr(keys), _ptr(w), _ptr(plane)), "bwtc_hip_test_code_keys")
        return keys[:n], w[:n], plane[:n]

    # the suffix sorter's finisher, launch by launch (bwtc_hip_test_finish_pass / _local_pass)
    def test_finish_pass(self, T, regions, S, P, H, C, window=1024, group=256, words=2, rounds=1, floor=12, out_n=None, lf_n=0,
                         rank=None, at=0, at2=0):
        """One k_finish launch over the list (S, P, H, C) in `regions` [(ebase, ecount), ...] of T as the sorter holds it;
        rank given: k_finish<RANK> with (rank, at, at2), then k_rank_updates.  -> dict: next (S, P, H, C arrays), next_base[16],
        next_count[17], hard / shallow (S, HP[, C]) cut to their counts, hard_count[2], shal_count[2], SA, out, pidx,
        last_char, lf[256] and, with ranks, us, ur, rank."""
        T = np.ascontiguousarray(T, dtype=np.uint8)
        n = T.size
        S, P, H = (np.ascontiguousarray(a, dtype=np.uint32) for a in (S, P, H))
        C = np.ascontiguousarray(C, dtype=np.uint16)
        ebase = np.array([r[0] for r in regions], np.uint32)
        ecount = np.array([r[1] for r in regions], np.uint32)
        span = int(max([0] + [b + c for b, c in regions]))
        assert S.size >= span and P.size >= span and H.size >= span and C.size >= span
        m = int(ecount.sum())
        stride = max(1, window - group)                      # (a shape the hook refuses still gets its arrays)
        grid = sum(-(-int(c) // stride) for c in ecount)
        room = grid * stride + -(-grid // 64) * group
        ranks = rank is not None
        p = FinPass()
        p.n, p.nreg, p.ebase, p.ecount = n, len(regions), _ptr(ebase), _ptr(ecount)
        p.S, p.P, p.H, p.C = _ptr(S), _ptr(P), _ptr(H), _ptr(C)
        p.window, p.group, p.words, p.rounds = int(window), int(group), int(words), int(rounds)
        p.floor, p.out_n, p.lf_n = int(floor), int(n if out_n is None else out_n), int(lf_n)
        p.lf_x = n // lf_n if lf_n > 1 else 0
        keep = dict(nS=np.zeros(room + 1, np.uint32), nP=np.zeros(room + 1, np.uint32), nH=np.zeros(room + 1, np.uint32), nC=np.zeros(room + 1, np.uint16),
                    next_base=np.zeros(16, np.uint32), next_count=np.zeros(17, np.uint32),
                    hS=np.zeros(m + 1, np.uint32), hHP=np.zeros(m + 1, np.uint64), hC=np.zeros(m + 1, np.uint16), hard_count=np.zeros(2, np.uint32),
                    sS=np.zeros(m + 1, np.uint32), sHP=np.zeros(m + 1, np.uint64), shal_count=np.zeros(2, np.uint32),
                    SA=np.zeros(n + 1, np.uint32), out=np.zeros(n + 1, np.uint8), small=np.zeros(2, np.uint32), lf=np.zeros(256, np.uint32))
        if ranks:
            keep.update(rank=np.array(rank, dtype=np.uint32), us=np.zeros(span + 1, np.uint32), ur=np.zeros(span + 1, np.uint32))
            assert keep["rank"].size == n
            p.at, p.at2 = int(at), int(at2)
        for k, a in keep.items():
            setattr(p, k, _ptr(a))
        p.next_cap = room
        fn = self.lib.bwtc_hip_test_local_pass if ranks else self.lib.bwtc_hip_test_finish_pass
        _check(fn(self.handle, _ptr(T) if n else None, ctypes.byref(p)), "bwtc_hip_test_local_pass" if ranks else "bwtc_hip_test_finish_pass")
        hc, sc = int(keep["hard_count"][0]), int(keep["shal_count"][0])
        res = dict(next=(keep["nS"][:room], keep["nP"][:room], keep["nH"][:room], keep["nC"][:room]), next_base=keep["next_base"],
                   next_count=keep["next_count"], hard=(keep["hS"][:hc], keep["hHP"][:hc], keep["hC"][:hc]), hard_count=keep["hard_count"],
                   shallow=(keep["sS"][:sc], keep["sHP"][:sc]), shal_count=keep["shal_count"], SA=keep["SA"][:n], out=keep["out"][:n],
                   pidx=int(keep["small"][0]), last_char=int(keep["small"][1]), lf=keep["lf"])
        if ranks:
            res.update(us=keep["us"][:span], ur=keep["ur"][:span], rank=keep["rank"])
        return res

    def test_finisher(self, T, S, P, H, C, window=1024, group=256, words=2, rounds=3, floor=12, keep_local=True, max_passes=8, out_n=None, lf_n=0):
        """finisher_passes over the one-region list (S, P, H, C) -> dict: hard, hard_depth, left, local (FinOutcome),
        passes_done, route, parked, park_holes, shallow_depth, wait_depth, local_depth, park / shallow (S, HP) and the local
        list (S, P, H, C) cut to their counts, SA, out, pidx, last_char, lf[256]."""
        T = np.ascontiguousarray(T, dtype=np.uint8)
        n = T.size
        S, P, H = (np.ascontiguousarray(a, dtype=np.uint32) for a in (S, P, H))
        C = np.ascontiguousarray(C, dtype=np.uint16)
        m = S.size
        assert P.size == m and H.size == m and C.size == m
        p = FinRun()
        p.n, p.m, p.S, p.P, p.H, p.C = n, m, _ptr(S), _ptr(P), _ptr(H), _ptr(C)
        p.window, p.group, p.words, p.rounds = int(window), int(group), int(words), int(rounds)
        p.floor, p.out_n, p.lf_n = int(floor), int(n if out_n is None else out_n), int(lf_n)
        p.lf_x = n // lf_n if lf_n > 1 else 0
        p.keep_local, p.max_passes = 1 if keep_local else 0, int(max_passes)
        keep = dict(outcome=np.zeros(4, np.uint32), info=np.zeros(8, np.uint32), pS=np.zeros(m + 1, np.uint32), pHP=np.zeros(m + 1, np.uint64),
                    sS=np.zeros(m + 1, np.uint32), sHP=np.zeros(m + 1, np.uint64), lS=np.zeros(m + 1, np.uint32), lP=np.zeros(m + 1, np.uint32),
                    lH=np.zeros(m + 1, np.uint32), lC=np.zeros(m + 1, np.uint16), SA=np.zeros(n + 1, np.uint32), out=np.zeros(n + 1, np.uint8),
                    small=np.zeros(2, np.uint32), lf=np.zeros(256, np.uint32))
        for k, a in keep.items():
            setattr(p, k, _ptr(a))
        _check(self.lib.bwtc_hip_test_finisher(self.handle, _ptr(T) if n else None, ctypes.byref(p)), "bwtc_hip_test_finisher")
        o, i = [int(v) for v in keep["outcome"]], [int(v) for v in keep["info"]]
        return dict(hard=o[0], hard_depth=o[1], left=o[2], local=o[3], passes_done=i[0], route=i[1], parked=i[2], park_holes=i[3], shallow=i[4],
                    shallow_depth=i[5], wait_depth=i[6], local_depth=i[7], park=(keep["pS"][:i[2]], keep["pHP"][:i[2]]),
                    shal=(keep["sS"][:i[4]], keep["sHP"][:i[4]]), local_list=(keep["lS"][:o[3]], keep["lP"][:o[3]], keep["lH"][:o[3]], keep["lC"][:o[3]]),
                    SA=keep["SA"][:n], out=keep["out"][:n], pidx=int(keep["small"][0]), last_char=int(keep["small"][1]), lf=keep["lf"])


    # the suffix sorter's ranking step and round kernels (bwtc_hip_test_rank_* / _round_keys)
    def test_rank_pass(self, T, keys, idx, m=None, init=True, split=False, mode=0, emit=0, w=None, aglob=None, short_len=0, kmask=None,
                       long=None, inv_lut=None, out_n=None, lf_n=0, rec_shift=0, plane=True):
        """One ranking (reduce, scan, apply) over the list (keys, idx[, w][, aglob]) of T as the sorter holds it.  keys: uint32
        or uint64; idx: uint32 suffix numbers, or with split their uint16 lower halves; long: dict(wmask, hi_shift, chr_shift,
        chr_mask, lvl_shift, depth) for long items (w given).  -> dict of every output array, cut to its size (aggA/B/C
        per tile, counts[2], rank[n], pair_s / pair_r / rec / val / rplane [m], aidx / aglob / agrp [m], achr (uint8[m], in
        mode 3 uint16[m]), SA, out, pidx, last_char, lf[256]); what the form does not write is still poison."""
        T = np.ascontiguousarray(T, dtype=np.uint8)
        n = T.size
        keys = np.ascontiguousarray(keys)
        assert keys.dtype in (np.uint32, np.uint64)
        idx = np.ascontiguousarray(idx, dtype=np.uint16 if split else np.uint32)
        m = keys.size if m is None else int(m)
        assert idx.size == keys.size
        p = RankPass()
        p.m, p.n, p.key_bytes, p.init, p.split, p.lng, p.mode, p.emit = m, n, keys.dtype.itemsize, int(bool(init)), int(bool(split)), int(w is not None), int(mode), int(emit)
        hold = [keys, idx]
        p.keys, p.idx = _ptr(keys), _ptr(idx)
        if w is not None:
            w = np.ascontiguousarray(w, dtype=np.uint32)
            assert w.size == keys.size
            hold.append(w)
            p.w = _ptr(w)
            p.wmask, p.hi_shift, p.chr_shift, p.chr_mask = int(long["wmask"]), int(long["hi_shift"]), int(long["chr_shift"]), int(long["chr_mask"])
            p.lvl_shift, p.depth = int(long["lvl_shift"]), int(long["depth"])
        if aglob is not None:
            aglob = np.ascontiguousarray(aglob, dtype=np.uint32)
            assert aglob.size == keys.size
            hold.append(aglob)
            p.aglob = _ptr(aglob)
        if inv_lut is not None:
            inv_lut = np.ascontiguousarray(inv_lut, dtype=np.uint8)
            assert inv_lut.size == 256
            hold.append(inv_lut)
            p.inv_lut = _ptr(inv_lut)
        p.short_len = int(short_len)
        p.kmask = int((1 << (8 * keys.dtype.itemsize)) - 1 if kmask is None else kmask)
        p.out_n, p.lf_n = int(n if out_n is None else out_n), int(lf_n)
        p.lf_x = n // lf_n if lf_n > 1 else 0
        p.rec_shift, p.plane = int(rec_shift), int(bool(plane))
        mm, tiles = max(m, 1), max(-(-m // 2048), 1)
        keep = dict(aggA=np.zeros(tiles, np.uint32), aggB=np.zeros(tiles, np.uint32), aggC=np.zeros(tiles, np.uint32), counts=np.zeros(2, np.uint32),
                    rank=np.zeros(n + 1, np.uint32), pair_s=np.zeros(mm, np.uint32), pair_r=np.zeros(mm, np.uint32), rec=np.zeros(mm, np.uint64),
                    val=np.zeros(mm, np.uint32), rplane=np.zeros(mm, np.uint8), aidx=np.zeros(mm, np.uint32), aglob_out=np.zeros(mm, np.uint32),
                    agrp=np.zeros(mm, np.uint32), achr=np.zeros(2 * mm, np.uint8), SA=np.zeros(n + 1, np.uint32), out=np.zeros(n + 1, np.uint8),
                    small=np.zeros(2, np.uint32), lf=np.zeros(256, np.uint32))
        for k, a in keep.items():
            setattr(p, k, _ptr(a))
        _check(self.lib.bwtc_hip_test_rank_pass(self.handle, _ptr(T) if n else None, ctypes.byref(p)), "bwtc_hip_test_rank_pass")
        res = dict(keep)
        res["rank"], res["SA"], res["out"] = keep["rank"][:n], keep["SA"][:n], keep["out"][:n]
        res["aglob"] = res.pop("aglob_out")
        res["achr"] = keep["achr"].view(np.uint16)[:mm] if mode == 3 else keep["achr"][:mm]
        res["pidx"], res["last_char"] = int(keep["small"][0]), int(keep["small"][1])
        return res

    def test_rank_scan(self, a, b, c, parts_cap=None):
        """k_rerank_scan_tiles<0> then <1> over three aggregate arrays -> (a, b, c scanned, the part array, counts[2])."""
        a, b, c = (np.array(x, dtype=np.uint32) for x in (a, b, c))
        nt = a.size
        assert b.size == nt and c.size == nt
        if parts_cap is None:
            parts_cap = 3 * (-(-nt // 4096)) + 3
        parts, counts = np.zeros(max(parts_cap, 1), np.uint32), np.zeros(2, np.uint32)
        _check(self.lib.bwtc_hip_test_rank_scan(self.handle, _ptr(a), _ptr(b), _ptr(c), nt, _ptr(parts), int(parts_cap), _ptr(counts)),
               "bwtc_hip_test_rank_scan")
        return a, b, c, parts[:parts_cap], counts

    def test_rank_scatter(self, rank, where=None, what=None, rec=None, bin_shift=0):
        """k_scatter_pairs (where, what) or k_scatter_dense (rec = s << 32 | value) into a copy of rank[] -> rank[] afterwards."""
        rank = np.array(rank, dtype=np.uint32)
        dense = rec is not None
        if dense:
            rec = np.ascontiguousarray(rec, dtype=np.uint64)
            m = rec.size
            args = (None, None, _ptr(rec) if m else None)
        else:
            where, what = np.ascontiguousarray(where, dtype=np.uint32), np.ascontiguousarray(what, dtype=np.uint32)
            m = where.size
            assert what.size == m
            args = (_ptr(where) if m else None, _ptr(what) if m else None, None)
        _check(self.lib.bwtc_hip_test_rank_scatter(self.handle, int(dense), args[0], args[1], args[2], m, rank.size, int(bin_shift), _ptr(rank)),
               "bwtc_hip_test_rank_scatter")
        return rank

    def test_round_keys(self, T, kind, h, bc, aidx=None, agrp=None, rec=None, val=None, rank=None, achr=None, emit=False, bin_shift=0,
                        run_mode=0, k=None, h_split=0, p=1):
        """One launch of k_gather_key2 (kind 0), k_gather_text (1) or k_gather_dense (2) -> keys, and for kind 2 (keys, vals)."""
        T = np.ascontiguousarray(T, dtype=np.uint8)
        q = RoundKeys()
        q.kind, q.n, q.h, q.bc, q.emit, q.bin_shift, q.run_mode, q.h_split, q.p = int(kind), T.size, int(h), int(bc), int(bool(emit)), int(bin_shift), int(run_mode), int(h_split), int(p)
        hold = []

        def give(name, a, dt, copy=False):
            if a is None:
                return None
            a = np.array(a, dtype=dt) if copy else np.ascontiguousarray(a, dtype=dt)
            hold.append(a)
            setattr(q, name, _ptr(a))
            return a
        if kind == 2:
            rec, val = give("rec", rec, np.uint64, True), give("val", val, np.uint32, True)
            m = rec.size
        else:
            aidx, agrp = give("aidx", aidx, np.uint32), give("agrp", agrp, np.uint32)
            m = aidx.size
            achr = give("achr", achr, np.uint8)
        give("rank", rank, np.uint32)
        give("k", k, np.uint32)
        q.m = m
        keys = np.zeros(max(m, 1), np.uint64)
        q.keys = _ptr(keys)
        _check(self.lib.bwtc_hip_test_round_keys(self.handle, _ptr(T) if T.size else None, ctypes.byref(q)), "bwtc_hip_test_round_keys")
        return (keys[:m], val[:m]) if kind == 2 else keys[:m]


    def test_round(self, T, ks, vs, aglob, rank, h_next, emit=False, text=False, carry_in=False, raw_out=False, run_mode=0, k=None, step_p=1,
                   step_depth=0, pairs_min=1 << 21, window_bits=16, out_n=None, lf_n=0):
        """rank_step<u64, false> once over the sorted list (ks, vs, aglob) -> dict: m, groups, carry, text_chars, ran_run,
        the next list (ks, vs cut to m; raw_out: vs the raw list's suffixes), aglob, grp, chr (uint8, raw_out uint16), rank,
        SA, out, pidx, last_char, lf."""
        T = np.ascontiguousarray(T, dtype=np.uint8)
        n = T.size
        ks, vs, aglob = np.ascontiguousarray(ks, dtype=np.uint64), np.ascontiguousarray(vs, dtype=np.uint32), np.ascontiguousarray(aglob, dtype=np.uint32)
        m = ks.size
        assert vs.size == m and aglob.size == m
        rank = np.array(rank, dtype=np.uint32)
        assert rank.size == n
        q = Round()
        q.m, q.n, q.ks, q.vs, q.aglob, q.rank, q.h_next = m, n, _ptr(ks), _ptr(vs), _ptr(aglob), _ptr(rank), int(h_next)
        q.emit, q.text, q.carry_in, q.raw_out, q.run_mode = int(bool(emit)), int(bool(text)), int(bool(carry_in)), int(bool(raw_out)), int(run_mode)
        if k is not None:
            k = np.ascontiguousarray(k, dtype=np.uint32)
            q.k = _ptr(k)
        q.step_p, q.step_depth, q.pairs_min, q.window_bits = int(step_p), int(step_depth), int(pairs_min), int(window_bits)
        q.out_n, q.lf_n = int(n if out_n is None else out_n), int(lf_n)
        q.lf_x = n // lf_n if lf_n > 1 else 0
        mm = max(m, 1)
        keep = dict(result=np.zeros(6, np.uint32), nks=np.zeros(mm, np.uint64), nvs=np.zeros(mm, np.uint32), naglob=np.zeros(mm, np.uint32),
                    ngrp=np.zeros(mm, np.uint32), nchr=np.zeros(2 * mm, np.uint8), SA=np.zeros(n + 1, np.uint32), out=np.zeros(n + 1, np.uint8),
                    small=np.zeros(2, np.uint32), lf=np.zeros(256, np.uint32))
        for name, a in keep.items():
            setattr(q, name, _ptr(a))
        _check(self.lib.bwtc_hip_test_round(self.handle, _ptr(T) if n else None, ctypes.byref(q)), "bwtc_hip_test_round")
        r = [int(v) for v in keep["result"]]
        cut = m if raw_out else r[0]
        return dict(m=r[0], groups=r[1], carry=bool(r[2]), text_chars=r[3], ran_run=bool(r[4]), finish=bool(r[5]), ks=keep["nks"][:r[0]],
                    vs=keep["nvs"][:cut], aglob=keep["naglob"][:m], grp=keep["ngrp"][:m],
                    chr=keep["nchr"].view(np.uint16)[:m] if raw_out else keep["nchr"][:m], rank=rank, SA=keep["SA"][:n], out=keep["out"][:n],
                    pidx=int(keep["small"][0]), last_char=int(keep["small"][1]), lf=keep["lf"])


def host_cpu_slice(numa_node, rank, ranks):
    """CPUs for the workers of context `rank` of `ranks` contexts that share NUMA node `numa_node`
    (-1: no node restriction): a contiguous slice of what this process may use.  Host only."""
    L = load()
    buf = np.zeros(4096, np.uint32)
    n = L.bwtc_hip_host_cpu_slice(int(numa_node), int(rank), int(ranks), _ptr(buf), buf.size)
    if n < 0:
        raise BwtcHipError("bwtc_hip_host_cpu_slice failed with code %d" % n)
    return [int(c) for c in buf[:n]]


def host_staging_bytes():
    """(now, peak) bytes of host staging memory this process holds for blocks under way."""
    L = load()
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    L.bwtc_hip_host_staging_bytes(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def _models_args(packed, tasks):
    return np.ascontiguousarray(packed, np.uint32), np.ascontiguousarray(tasks, np.uint32).reshape(-1, 3)


def host_test_models(packed, n_coded, tasks, state_in, letter="B"):
    """The model passes lane by lane on the host over given packed streams and tasks (bwtc_hip_host_test_models, for
    another main model than 'B' bwtc_hip_host_test_models_letter; no device): (w, state after the block)."""
    packed, tasks = _models_args(packed, tasks)
    w = np.zeros(int(n_coded), np.uint16)
    st = _u32(0)
    if letter == "B":
        _check(load().bwtc_hip_host_test_models(_ptr(packed), int(n_coded), _ptr(tasks), tasks.shape[0], state_in, _ptr(w),
                                                ctypes.byref(st)), "bwtc_hip_host_test_models")
    else:
        _check(load().bwtc_hip_host_test_models_letter(letter.encode(), _ptr(packed), int(n_coded), _ptr(tasks), tasks.shape[0], state_in,
                                                       _ptr(w), ctypes.byref(st)), "bwtc_hip_host_test_models_letter")
    return w, st.value


def host_wavelet_elements(section_args, state, letter="B"):
    """The coded elements of a real block, from the section-run arguments of bwtc_hip_host_wavelet_streams (a tuple of
    n_sections and seven arrays): (packed codes, n_coded, tasks [(begin, end, type)], w of the sequential host coder,
    state after the block) -- bwtc_hip_host_wavelet_elements, for another main model than 'B' ..._elements_letter."""
    L = load()
    if letter == "B":
        elements = L.bwtc_hip_host_wavelet_elements
    else:
        def elements(*a):
            return L.bwtc_hip_host_wavelet_elements_letter(letter.encode(), *a)
    nsec, arrays = section_args[0], [np.ascontiguousarray(a) for a in section_args[1:]]
    ptrs = [_ptr(a) for a in arrays]
    n, nt = _u32(0), _u32(0)
    st = _u32(state)
    _check(elements(nsec, *ptrs, ctypes.byref(st), ctypes.byref(n), ctypes.byref(nt), None, 0, None, 0, None, 0),
           "bwtc_hip_host_wavelet_elements")
    packed = np.zeros((n.value + 15) // 16, np.uint32)
    tasks = np.zeros((nt.value, 3), np.uint32)
    w = np.zeros(n.value, np.uint16)
    st = _u32(state)
    _check(elements(nsec, *ptrs, ctypes.byref(st), ctypes.byref(n), ctypes.byref(nt), _ptr(packed), packed.size,
                    _ptr(tasks), tasks.shape[0], _ptr(w), w.size), "bwtc_hip_host_wavelet_elements")
    return packed, n.value, tasks, w, st.value


def synth_into(kind, seed, out):
    """Fills the uint8 array `out` with the synthetic block of `kind` ('r', 'd', 't') and `seed`:
    the library's C++ generator, the same bytes as bwtc_amd.synth (tests/test_abi.py)."""
    _check(load().bwtc_hip_synth(kind.encode(), seed, out.size, _ptr(out)), "bwtc_hip_synth")
    return out
