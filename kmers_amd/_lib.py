"""ctypes binding of the libkmx C ABI (include/kmx.h).

There is deliberately NO fallback: if libkmx.so is missing, or no HIP device is visible when
a context is created, this raises.  The CPU oracle under oracle/ is test infrastructure and
is never imported from here.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# The one library this package loads.  Nothing in the environment changes it: development builds (tools/dev_variant.py) are
# selected by the tool or test that wants one (tools/devlib.py, `pytest --kmx-lib`), in code, before load().
LIB_PATH = os.path.join(_HERE, "libkmx.so")
COMM_ID_BYTES = 128

# status codes (include/kmx.h)
OK, E_ARG, E_K_RANGE, E_HIP, E_INVALID_BASE, E_TOO_LONG, E_NOMEM = range(7)
HASH_NONE, HASH_LEX, HASH_IDENTITY = 0, 1, 2
NO_MATCH, IDENTITY_MATCH, TWIN_MATCH = 0, 1, 2
WIN_VALID, WIN_FW_CANONICAL = 1, 2
REDUCE_SUM_FW = 1
# kmx_count_setop(2): the operation, and the count of a key both tables hold (INTERSECT and UNION)
SETOP_INTERSECT, SETOP_UNION, SETOP_SUBTRACT, SETOP_SYMDIFF, SETOP_COUNTER_SUBTRACT = range(5)
RULE_SUM, RULE_MIN, RULE_MAX, RULE_LEFT, RULE_RIGHT = range(5)
# merged entries per tile of kmx_count_setop(2) / kmx_count_compare(2) (kmx_count_setop.hip: SETOP_TILE): where the boundary tests
# put their shared keys, and what the documented working set counts in
SETOP_TILE = 2048
# kmx_count_read_stats(2): the words of a read's row
RS_N_VALID, RS_N_PRESENT, RS_N_SOLID, RS_MIN, RS_MAX, RS_SUM, RS_MEDIAN, RS_SPAN = range(8)
RS_WORDS = 8
# kmx_count_correct_reads(2): the words of a read's row
CR_N_WEAK, CR_N_CANDIDATES, CR_N_CORRECTED, CR_N_AMBIGUOUS = range(4)
CR_WORDS = 4
# kmx_count_read_colors(2): the words of a read's row
RC_N_VALID, RC_N_HIT, RC_N_UNIQUE, RC_ALL, RC_ANY, RC_THRESH, RC_BEST, RC_N_SWITCH = range(8)
RC_WORDS = 8
# kmx_count_adjacency(2): the word of d_nbr where an edge is absent (KMX_NO_ENTRY; -1 in the int64 tensors of kmers_amd.api)
NO_ENTRY = 2**64 - 1
# kmx_count_unitig_index / kmx_count_read_paths(2): an entry in no unitig, and the words of a segment's record
PLACE_NONE = 0
PATH_READ, PATH_SPAN, PATH_UNITIG, PATH_POS = range(4)
PATH_WORDS = 4
# kmx_count_unitig_clean: why a unitig is dropped (KMX_CLEAN_*; 0 = kept)
CLEAN_KEEP, CLEAN_TIP, CLEAN_BUBBLE, CLEAN_ISLAND = range(4)
# kmx_count_unitig_components: the label and id of a unitig the mask leaves out (KMX_COMPONENT_NONE; -1 in the int64 tensors of
# kmers_amd.api), and the words of a component's record
COMPONENT_NONE = 2**64 - 1
COMP_ROOT, COMP_N_UNITIGS, COMP_N_NODES, COMP_COUNT_SUM = range(4)
COMP_WORDS = 4
# kmx_count_link_support: the words of the summary (KMX_LS_*)
LS_JUNCTIONS, LS_CROSSED, LS_UNLINKED = range(3)
LS_WORDS = 3
# kmx_reads_quality: the words of a read's row (KMX_RQ_*)
RQ_BASES, RQ_LOW, RQ_QSUM, RQ_WEIGHT, RQ_MINMAX, RQ_TRIM, RQ_RUN, RQ_WINDOWS = range(8)
RQ_WORDS = 8
# kmx_reads_adapter / kmx_reads_pair_overlap: the words of a row (KMX_RA_* / KMX_RP_*), the limits
RA_KEEP, RA_HIT, RA_BASES, RA_HITS = range(4)
RA_WORDS = 4
RA_MAX_ADAPTERS, RA_MAX_ADAPTER_LEN = 8, 64
RP_INSERT, RP_OVERLAP, RP_KEEP1, RP_KEEP2 = range(4)
RP_WORDS = 4
RP_MAX_LEN = 1024
# kmx_reads_complexity: the words of a read's row (KMX_RX_*)
RX_KEEP, RX_BASES, RX_TAIL, RX_HEAD, RX_AC, RX_GT, RX_DIFF, RX_DUST = range(8)
RX_WORDS = 8
RX_DUST_NEVER = 1891   # a dust_max no window exceeds: the numerator of a full window of one letter
# kmx_reads_pair_merge: the words of a pair's row (KMX_RM_*)
RM_LEN, RM_OVERLAP, RM_TAKEN, RM_INVALID = range(4)
RM_WORDS = 4
# kmx_reads_dedup: the flag, the words of an item's row, the bits of its flags word and the words of the summary (KMX_DD_*)
DD_STRAND = 1
DD_REP, DD_COUNT, DD_FLAGS, DD_HASH = range(4)
DD_WORDS = 4
DD_F_KEPT, DD_F_FLIPPED, DD_F_COLLISION, DD_F_OTHER = 1, 2, 4, 8
DD_S_KEPT, DD_S_DROPPED, DD_S_LARGEST, DD_S_COLLISIONS = range(4)
DD_SUMMARY_WORDS = 4
# kmx_sketch_*: a block's bytes, the largest log2_blocks, and the lanes per compute unit of one grid sweep of the add, lookup and
# filter kernels (kmx_sketch.hip: SKETCH_BLOCKS_PER_CU blocks of 256 -- where the tests put their "more than one sweep")
SKETCH_BLOCK_BYTES = 64
SKETCH_MAX_LOG2_BLOCKS = 32
SKETCH_SWEEP_LANES_PER_CU = 1024
# kmx_hll_*: the range of log2_regs, the bins of one array of kmx_hll_stats, and the cut-over of the add kernel (kmx_hll.hip:
# block-private LDS registers up to HLL_LDS_MAX_LOG2_REGS, once every block of the sweep has HLL_LDS_KEYS_PER_DWORD keys for each
# dword it flushes -- where the tests put their keys to run both routes)
HLL_MIN_LOG2_REGS = 4
HLL_MAX_LOG2_REGS = 24
HLL_BINS = 64
HLL_LDS_MAX_LOG2_REGS = 14
HLL_LDS_KEYS_PER_DWORD = 1


class KmxError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"kmx status {status}: {msg}")
        self.status = status


class Reads(C.Structure):
    _fields_ = [("d_bases", C.c_void_p), ("n_reads", C.c_uint64), ("read_len", C.c_uint32), ("d_offsets", C.c_void_p)]


class Summary(C.Structure):
    _fields_ = [("n_valid", C.c_uint64), ("sum_canon", C.c_uint64), ("xor_hash", C.c_uint64), ("sum_fw", C.c_uint64)]


class Summary2(C.Structure):
    _fields_ = [("n_valid", C.c_uint64), ("sum_lo", C.c_uint64), ("sum_hi", C.c_uint64), ("xor_lo", C.c_uint64),
                ("xor_hi", C.c_uint64)]


class TableCompare(C.Structure):
    """kmx_table_compare: what kmx_count_compare(2) fills"""
    _fields_ = [(n, C.c_uint64) for n in ("n_both", "n_only_a", "n_only_b", "sum_a", "sum_b", "sum_a_both", "sum_b_both", "sum_min",
                                          "sum_max")]


_vp, _u64, _u32, _u8, _int = C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint8, C.c_int
_RP = C.POINTER(Reads)

# every symbol include/kmx.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "kmx_version": (_int, []),
    "kmx_strerror": (C.c_char_p, [_int]),
    "kmx_ctx_create": (_int, [_int, C.POINTER(_vp)]),
    "kmx_ctx_create_on_stream": (_int, [_int, _vp, C.POINTER(_vp)]),
    "kmx_ctx_destroy": (None, [_vp]),
    "kmx_ctx_synchronize": (_int, [_vp]),
    "kmx_ctx_device": (_int, [_vp]),
    "kmx_ctx_set_work_buffer_limit": (_int, [_vp, C.c_size_t]),
    "kmx_ctx_work_buffer_info": (_int, [_vp, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]),
    "kmx_last_error": (C.c_char_p, [_vp]),
    "kmx_malloc": (_int, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "kmx_free": (_int, [_vp, _vp]),
    "kmx_memcpy_h2d": (_int, [_vp, _vp, _vp, C.c_size_t]),
    "kmx_memcpy_d2h": (_int, [_vp, _vp, _vp, C.c_size_t]),
    "kmx_memset": (_int, [_vp, _vp, _int, C.c_size_t]),
    "kmx_canonical_reduce": (_int, [_vp, _RP, _u32, _u32, _u32, _u32, _vp]),
    "kmx_canonical_reduce_host": (_int, [_vp, _RP, _u32, _u32, _u32, _u32, _vp]),
    "kmx_canonical_windows": (_int, [_vp, _RP, _vp, _u32, _vp, _vp, _vp, _vp]),
    "kmx_canonical_reduce2": (_int, [_vp, _RP, _u32, _u32, _vp]),
    "kmx_canonical_windows2": (_int, [_vp, _RP, _vp, _u32, _vp, _vp, _vp, _vp]),
    "kmx_histogram": (_int, [_vp, _RP, _u32, _u32, _u32, _u32, _vp]),
    "kmx_gen_reads": (_int, [_vp, _u64, _u64, _vp, _u64]),
    "kmx_kmers_from_bytes": (_int, [_vp, _vp, _u64, _u32, _vp, C.POINTER(_u64)]),
    "kmx_revcomp_words": (_int, [_vp, _vp, _u64, _u32, _vp]),
    "kmx_canonical_words": (_int, [_vp, _vp, _u64, _u32, _vp, _vp]),
    "kmx_hash_words": (_int, [_vp, _vp, _u64, _u32, _u32, _vp]),
    "kmx_hash_words_sip13": (_int, [_vp, _vp, _u64, _u64, _u64, _vp]),
    "kmx_match_words": (_int, [_vp, _vp, _vp, _vp, _u64, _vp]),
    "kmx_ck_append_bases": (_int, [_vp, _vp, _vp, _vp, _u64, _u32, _vp]),
    "kmx_ck_prepend_bases": (_int, [_vp, _vp, _vp, _vp, _u64, _u32, _vp]),
    "kmx_encode_kmers": (_int, [_vp, _vp, _u64, _u32, _u8, _u32, _vp]),
    "kmx_encode_windows": (_int, [_vp, _RP, _u32, _u8, _u32, _vp]),
    "kmx_encoding_rev_comp": (_int, [_vp, _vp, _u64, _u32, _u8, _u32, _vp]),
    "kmx_encoding_decode": (_int, [_vp, _vp, _u64, _u8, _u32, _vp]),
    "kmx_seqvec_push_chars": (_int, [_vp, _vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    "kmx_seqvec_to_bytes": (_int, [_vp, _vp, _u64, _vp]),
    "kmx_seqvec_get_kmers": (_int, [_vp, _vp, _u64, _vp, _u64, _u32, _vp]),
    "kmx_seqvec_iter_kmers": (_int, [_vp, _vp, _u64, _u64, _u64, _u32, _vp]),
    "kmx_seqvec_canonical_reduce": (_int, [_vp, _vp, _u64, _u32, _u32, _u32, _u32, _u32, _vp]),
    "kmx_minimizer_words": (_int, [_vp, _vp, _u64, _u32, _u32, _u32, _u32, _vp, _vp]),
    "kmx_seqvec_minimizers": (_int, [_vp, _vp, _u64, _u32, _u32, _u32, _u32, _u32, _vp, _vp]),
    "kmx_minimizers": (_int, [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    "kmx_canonical_reduce_sip13": (_int, [_vp, _RP, _u32, _u64, _u64, _u32, _vp]),
    "kmx_histogram_sip13": (_int, [_vp, _RP, _u32, _u64, _u64, _u32, _vp]),
    "kmx_count_canonical": (_int, [_vp, _RP, _u32, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "kmx_count_merge": (_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "kmx_count_canonical2": (_int, [_vp, _RP, _u32, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "kmx_count_merge2": (_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "kmx_sketch_add_words": (_int, [_vp, _vp, _vp, _u64, _vp, _u32, _u64]),
    "kmx_sketch_add_words2": (_int, [_vp, _vp, _vp, _u64, _vp, _u32, _u64]),
    "kmx_sketch_add": (_int, [_vp, _RP, _u32, _vp, _u32, _u64]),
    "kmx_sketch_add2": (_int, [_vp, _RP, _u32, _vp, _u32, _u64]),
    "kmx_sketch_lookup": (_int, [_vp, _vp, _u64, _vp, _u32, _u64, _vp]),
    "kmx_sketch_lookup2": (_int, [_vp, _vp, _u64, _vp, _u32, _u64, _vp]),
    "kmx_sketch_lookup_reads": (_int, [_vp, _RP, _vp, _u32, _vp, _u32, _u64, _vp]),
    "kmx_sketch_lookup_reads2": (_int, [_vp, _RP, _vp, _u32, _vp, _u32, _u64, _vp]),
    "kmx_sketch_merge": (_int, [_vp, _vp, _vp, _u32, _vp]),
    "kmx_sketch_stats": (_int, [_vp, _vp, _u32, _vp]),
    "kmx_hll_add_words": (_int, [_vp, _vp, _u64, _vp, _u32, _u64]),
    "kmx_hll_add_words2": (_int, [_vp, _vp, _u64, _vp, _u32, _u64]),
    "kmx_hll_add": (_int, [_vp, _RP, _u32, _vp, _u32, _u64]),
    "kmx_hll_add2": (_int, [_vp, _RP, _u32, _vp, _u32, _u64]),
    "kmx_hll_merge": (_int, [_vp, _vp, _vp, _u32, _vp]),
    "kmx_hll_stats": (_int, [_vp, _vp, _vp, _u32, _vp]),
    "kmx_count_canonical_min": (_int, [_vp, _RP, _u32, _vp, _u32, _u64, _u32, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "kmx_count_canonical_min2": (_int, [_vp, _RP, _u32, _vp, _u32, _u64, _u32, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "kmx_count_lookup": (_int, [_vp, _vp, _vp, _u64, _u32, _vp, _vp, _u64, _vp]),
    "kmx_count_lookup2": (_int, [_vp, _vp, _vp, _u64, _u32, _vp, _vp, _u64, _vp]),
    "kmx_count_lookup_reads": (_int, [_vp, _RP, _vp, _u32, _vp, _vp, _u64, _vp]),
    "kmx_count_lookup_reads2": (_int, [_vp, _RP, _vp, _u32, _vp, _vp, _u64, _vp]),
    "kmx_count_read_stats": (_int, [_vp, _RP, _u32, _vp, _vp, _u64, _u64, _vp]),
    "kmx_count_read_stats2": (_int, [_vp, _RP, _u32, _vp, _vp, _u64, _u64, _vp]),
    "kmx_count_correct_reads": (_int, [_vp, _RP, _u32, _vp, _vp, _u64, _u64, _u32, _vp, _vp]),
    "kmx_count_correct_reads2": (_int, [_vp, _RP, _u32, _vp, _vp, _u64, _u64, _u32, _vp, _vp]),
    "kmx_count_color_matrix": (_int, [_vp, _vp, _u64, _u32, _vp, _vp]),
    "kmx_count_read_colors": (_int, [_vp, _RP, _u32, _vp, _vp, _u64, _u32, _u32, _u32, _vp, _vp]),
    "kmx_count_read_colors2": (_int, [_vp, _RP, _u32, _vp, _vp, _u64, _u32, _u32, _u32, _vp, _vp]),
    "kmx_count_spectrum": (_int, [_vp, _vp, _u64, _u64, _vp]),
    "kmx_count_filter": (_int, [_vp, _vp, _vp, _u64, _u64, _u64, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "kmx_count_filter2": (_int, [_vp, _vp, _vp, _u64, _u64, _u64, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "kmx_count_adjacency": (_int, [_vp, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp]),
    "kmx_count_adjacency2": (_int, [_vp, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp]),
    "kmx_count_edge_histogram": (_int, [_vp, _vp, _u64, _vp]),
    "kmx_count_unitig_ends": (_int, [_vp, _vp, _vp, _vp, _u64, _vp]),
    "kmx_count_unitigs": (_int, [_vp, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kmx_count_unitigs2": (_int, [_vp, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kmx_count_unitig_sequences": (_int, [_vp, _vp, _u64, _u32, _vp, _vp, _u64, _vp]),
    "kmx_count_unitig_sequences2": (_int, [_vp, _vp, _u64, _u32, _vp, _vp, _u64, _vp]),
    "kmx_count_unitig_index": (_int, [_vp, _vp, _vp, _u64, _u64, _vp]),
    "kmx_count_read_paths": (_int, [_vp, _RP, _u32, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "kmx_count_read_paths2": (_int, [_vp, _RP, _u32, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "kmx_count_unitig_links": (_int, [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "kmx_count_unitig_select": (_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "kmx_count_unitig_select2": (_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "kmx_count_unitig_clean": (_int, [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _u64, _u32, _u32, _u64, _u64, _u64, _vp, _vp]),
    "kmx_count_unitig_components": (_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "kmx_count_link_support": (_int, [_vp, _vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp, _vp]),
    "kmx_count_adjacency_cut": (_int, [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp]),
    "kmx_reads_select": (_int, [_vp, _RP, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp, _u64, _u64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kmx_reads_gather": (_int, [_vp, _RP, _vp, _u64, _vp, _u64, _u32, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "kmx_count_setop": (_int, [_vp, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "kmx_count_setop2": (_int, [_vp, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "kmx_count_compare": (_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp]),
    "kmx_count_compare2": (_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp]),
    "kmx_minimizer_words_sip13": (_int, [_vp, _vp, _u64, _u32, _u32, _u64, _u64, _vp, _vp]),
    "kmx_seqvec_minimizers_sip13": (_int, [_vp, _vp, _u64, _u32, _u32, _u32, _u64, _u64, _vp, _vp]),
    "kmx_minimizers_sip13": (_int, [_vp, _RP, _vp, _u32, _u32, _u64, _u64, _vp, _vp, C.POINTER(C.c_uint64)]),
    "kmx_fastx_parse": (_int, [_vp, _vp, _u64, _u32, _vp, _vp, _u64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kmx_fastx_parse_quals": (_int, [_vp, _vp, _u64, _u32, _vp, _vp, _u64, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kmx_fastx_parse_names": (_int, [_vp, _vp, _u64, _u32, _vp, _vp, _u64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kmx_bgzf_index": (_int, [_vp, _vp, _u64, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "kmx_bgzf_inflate": (_int, [_vp, _vp, _u64, _vp, _vp, _u64, _u32, _vp, _u64, _vp, C.POINTER(C.c_uint64)]),
    "kmx_bgzf_deflate_bound": (_u64, [_u64, _u32]),
    "kmx_bgzf_deflate": (_int, [_vp, _vp, _u64, _u32, _u32, _vp, _u64, _vp, C.POINTER(C.c_uint64)]),
    "kmx_fastx_format": (_int, [_vp, C.POINTER(Reads), _vp, C.POINTER(Reads), _u32, _u64, _u32, _u32, _u32, _vp, _vp, _u64, C.POINTER(C.c_uint64)]),
    "kmx_reads_quality": (_int, [_vp, _RP, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    "kmx_reads_adapter": (_int, [_vp, _RP, _vp, _vp, _u32, _u32, _u32, _u32, _vp]),
    "kmx_reads_pair_overlap": (_int, [_vp, _RP, _RP, _u32, _u32, _u32, _u32, _vp]),
    "kmx_reads_complexity": (_int, [_vp, _RP, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp]),
    "kmx_reads_pair_merge": (_int, [_vp, _RP, _RP, _vp, _vp, _vp, _u64, _u32, _u32, _vp, _vp, _vp, _vp, _u64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kmx_reads_dedup": (_int, [_vp, _RP, _RP, _u32, _u32, _vp, _u64, _vp, _vp, C.POINTER(C.c_uint64)]),
    "kmx_sub_kmer_words": (_int, [_vp, _vp, _u64, _u32, _u32, _u32, _vp]),
    "kmx_kmers_to_strings": (_int, [_vp, _vp, _u64, _u32, _vp]),
    "kmx_bitmers_to_bytes": (_int, [_vp, _vp, _u64, _u32, _vp]),
    "kmx_encode_kmers_p": (_int, [_vp, _vp, _u64, _u32, _u8, _u32, _u32, _vp]),
    "kmx_encoding_rev_comp_p": (_int, [_vp, _vp, _u64, _u32, _u8, _u32, _u32, _vp]),
    "kmx_encoding_decode_p": (_int, [_vp, _vp, _u64, _u8, _u32, _u32, _vp]),
    "kmx_comm_get_unique_id": (_int, [_vp]),
    "kmx_comm_create": (_int, [_vp, _vp, _int, _int, C.POINTER(_vp)]),
    "kmx_comm_destroy": (None, [_vp]),
    "kmx_comm_size": (_int, [_vp]),
    "kmx_comm_rank": (_int, [_vp]),
    "kmx_histogram_allreduce": (_int, [_vp, _vp, _u64]),
    "kmx_summary_allreduce": (_int, [_vp, _vp]),
    "kmx_calib_stream_read": (_int, [_vp, _vp, _u64, _vp]),
    "kmx_reads_length_range": (_int, [_vp, _vp, _u64, _vp, _vp]),
}

FASTX_AUTO, FASTX_FASTQ, FASTX_FASTA = 0, 1, 2
FASTX_SAME_TEXT = 0x100   # or-ed into the format of the emit call that follows the counting call on the same image

BGZF_NO_CRC = 1   # kmx_bgzf_inflate flags: the CRC-32 of the blocks is not compared
BGZF_DEFLATE_STORED = 1   # kmx_bgzf_deflate flags: every block a stored block (level 0)
# KMX_BGZF_ST_*: why a block is not sound (d_status of kmx_bgzf_inflate)
BGZF_ST_HEADER, BGZF_ST_BTYPE, BGZF_ST_STORED, BGZF_ST_COUNTS, BGZF_ST_REPEAT, BGZF_ST_NO_EOB, BGZF_ST_CODESET, BGZF_ST_BADCODE, BGZF_ST_SYMBOL, \
    BGZF_ST_DISTANCE, BGZF_ST_OUTPUT, BGZF_ST_INPUT, BGZF_ST_LENGTH, BGZF_ST_CRC = range(1, 15)
BGZF_ST_NAMES = {0: "sound", BGZF_ST_HEADER: "block header", BGZF_ST_BTYPE: "DEFLATE block type 3", BGZF_ST_STORED: "stored block length",
                 BGZF_ST_COUNTS: "HLIT / HDIST out of range", BGZF_ST_REPEAT: "code-length repeat", BGZF_ST_NO_EOB: "no end-of-block code",
                 BGZF_ST_CODESET: "code-length set over-subscribed or incomplete", BGZF_ST_BADCODE: "bit pattern that is no code",
                 BGZF_ST_SYMBOL: "invalid length or distance symbol", BGZF_ST_DISTANCE: "distance too far back",
                 BGZF_ST_OUTPUT: "output passes ISIZE", BGZF_ST_INPUT: "input runs out", BGZF_ST_LENGTH: "length differs from ISIZE",
                 BGZF_ST_CRC: "CRC-32 mismatch"}

_LIB = None


def load(import_torch_first: bool = True):
    """dlopen kmers_amd/libkmx.so.  torch (if installed) is imported first so that libkmx's
    libamdhip64.so.7 dependency resolves to the HIP runtime torch already loaded -- two HIP
    runtimes in one process would not share device allocations."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -m kmers_amd.build` (hipcc, gfx950). "
            "kmers_amd has no CPU fallback.")
    if import_torch_first:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here == ABI mismatch with include/kmx.h
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def check(lib, ctx, status: int):
    if status == OK:
        return
    msg = lib.kmx_strerror(status).decode()
    if status == E_HIP and ctx:
        msg += " -- " + lib.kmx_last_error(ctx).decode()
    raise KmxError(status, msg)
