"""ctypes binding of the C ABI in include/pll.h + include/pllhip.h, and the
synthetic workload generator shared by tests/ and bench.py.

The binding is deliberately thin: it mirrors the C structs field by field
(`pll_partition_t`, `pll_operation_t`, `pll_unode_t`, `pll_utree_t`) and calls
the exported functions with plain pointers and sizes, i.e. exactly what a C
caller such as pll-modules' treeinfo.c does.  `PllLib(path)` can wrap any
shared library that exports the interface; this module itself only knows where
the PRODUCT library lives (`PRODUCT_LIB`).  The CPU oracle is loaded by tests/
and by bench.py's cpu_baseline leg, never from here.

Workloads follow SURVEY.md section 8d: splitmix64-seeded random stepwise-addition
tree (seed 42), branch lengths U(0.01, 0.2) (seed 43), iid uniform tip states
(seed 44), DNA GTR+G4 / "LG-shaped" protein / GY94-shaped codon models.
"""
import ctypes as C
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PRODUCT_LIB = os.path.join(HERE, "libpll_hip.so")

PLL_SCALE_BUFFER_NONE = -1
PLL_ATTRIB_PATTERN_TIP = 1 << 4
PLL_ATTRIB_AB_LEWIS, PLL_ATTRIB_AB_FELSENSTEIN, PLL_ATTRIB_AB_STAMATAKIS = 1 << 5, 2 << 5, 3 << 5
PLL_ATTRIB_AB_FLAG = 1 << 8
PLL_ATTRIB_RATE_SCALERS = 1 << 9
PLL_ATTRIB_SITE_REPEATS = 1 << 10
PLL_GAMMA_RATES_MEAN = 0
PLL_TREE_TRAVERSE_POSTORDER = 1
PLLHIP_SYNC_PMATRIX, PLLHIP_SYNC_CLV, PLLHIP_SYNC_SCALERS, PLLHIP_SYNC_TIPS, PLLHIP_SYNC_ALL = 1, 2, 4, 8, 15
PLLHIP_ATTRIB_HOST_MIRRORS = 1 << 30

c_double_p = C.POINTER(C.c_double)
c_uint_p = C.POINTER(C.c_uint)


class Repeats(C.Structure):
    """pll_repeats_t (include/pll.h): what pll-modules dereferences under PLL_ATTRIB_SITE_REPEATS"""
    _fields_ = [("pernode_site_id", C.POINTER(c_uint_p)), ("pernode_id_site", C.POINTER(c_uint_p)),
                ("pernode_ids", c_uint_p), ("perscale_ids", c_uint_p), ("pernode_allocated_clvs", c_uint_p),
                ("enable_repeats", C.c_void_p), ("reallocate_repeats", C.c_void_p)]


class Partition(C.Structure):
    _fields_ = [
        ("tips", C.c_uint), ("clv_buffers", C.c_uint), ("nodes", C.c_uint),
        ("states", C.c_uint), ("sites", C.c_uint), ("pattern_weight_sum", C.c_uint),
        ("rate_matrices", C.c_uint), ("prob_matrices", C.c_uint), ("rate_cats", C.c_uint),
        ("scale_buffers", C.c_uint), ("attributes", C.c_uint),
        ("alignment", C.c_size_t), ("states_padded", C.c_uint),
        ("clv", C.POINTER(c_double_p)), ("pmatrix", C.POINTER(c_double_p)),
        ("rates", c_double_p), ("rate_weights", c_double_p),
        ("subst_params", C.POINTER(c_double_p)),
        ("scale_buffer", C.POINTER(c_uint_p)),
        ("frequencies", C.POINTER(c_double_p)),
        ("prop_invar", c_double_p), ("invariant", C.POINTER(C.c_int)),
        ("pattern_weights", c_uint_p),
        ("eigen_decomp_valid", C.POINTER(C.c_int)),
        ("eigenvecs", C.POINTER(c_double_p)), ("inv_eigenvecs", C.POINTER(c_double_p)),
        ("eigenvals", C.POINTER(c_double_p)),
        ("maxstates", C.c_uint), ("tipchars", C.POINTER(C.POINTER(C.c_ubyte))),
        ("charmap", C.POINTER(C.c_ubyte)), ("ttlookup", c_double_p),
        ("tipmap", C.POINTER(C.c_ulonglong)),
        ("asc_bias_alloc", C.c_int), ("asc_additional_sites", C.c_int),
        ("repeats", C.POINTER(Repeats)), ("engine", C.c_void_p),
    ]


class Operation(C.Structure):
    _fields_ = [
        ("parent_clv_index", C.c_uint), ("parent_scaler_index", C.c_int),
        ("child1_clv_index", C.c_uint), ("child1_matrix_index", C.c_uint),
        ("child1_scaler_index", C.c_int),
        ("child2_clv_index", C.c_uint), ("child2_matrix_index", C.c_uint),
        ("child2_scaler_index", C.c_int),
    ]


class UNode(C.Structure):
    pass


UNode._fields_ = [
    ("label", C.c_char_p), ("length", C.c_double), ("node_index", C.c_uint),
    ("clv_index", C.c_uint), ("scaler_index", C.c_int), ("pmatrix_index", C.c_uint),
    ("next", C.POINTER(UNode)), ("back", C.POINTER(UNode)), ("data", C.c_void_p),
]


class UTree(C.Structure):
    _fields_ = [
        ("tip_count", C.c_uint), ("inner_count", C.c_uint), ("edge_count", C.c_uint),
        ("binary", C.c_int), ("nodes", C.POINTER(C.POINTER(UNode))),
        ("vroot", C.POINTER(UNode)),
    ]


class Counters(C.Structure):
    _fields_ = [(n, C.c_ulonglong) for n in (
        "partial_ops", "partial_launches", "site_updates", "pmatrix_updates", "pmatrix_launches",
        "lnl_calls", "sumtable_calls", "derivative_calls", "derivative_points", "model_uploads")]


class RepeatStats(C.Structure):
    _fields_ = [(n, C.c_ulonglong) for n in ("cherries", "classes", "sites", "expansions")]


class TransientStats(C.Structure):
    _fields_ = [(n, C.c_ulonglong) for n in ("skipped", "materialized", "discarded")]


class DeferredStats(C.Structure):
    _fields_ = [(n, C.c_ulonglong) for n in ("deferred", "stored_later", "given_up")]


class ScheduleStats(C.Structure):
    _fields_ = [(n, C.c_uint) for n in ("chains", "operations", "inner_reads", "folded_cherries", "lookup_children")]


class Profile(C.Structure):
    _fields_ = [("launches", C.c_ulonglong), ("ops", C.c_ulonglong),
                ("kernel_ms", C.c_double), ("algorithmic_bytes", C.c_double),
                ("algorithmic_flops", C.c_double), ("minimum_bytes", C.c_double)]


class Msa(C.Structure):
    """pll_msa_t"""
    _fields_ = [("count", C.c_int), ("length", C.c_int), ("sequence", C.POINTER(C.c_void_p)),
                ("label", C.POINTER(C.c_char_p))]


class MsaStats(C.Structure):
    """pllhip_msa_stats_t (the fields of pllmod_msa_stats_t)"""
    _fields_ = [("states", C.c_uint),
                ("dup_taxa_pairs_count", C.c_ulong), ("dup_taxa_pairs", C.POINTER(C.c_ulong)),
                ("dup_seqs_pairs_count", C.c_ulong), ("dup_seqs_pairs", C.POINTER(C.c_ulong)),
                ("gap_prop", C.c_double),
                ("gap_seqs_count", C.c_ulong), ("gap_seqs", C.POINTER(C.c_ulong)),
                ("gap_cols_count", C.c_ulong), ("gap_cols", C.POINTER(C.c_ulong)),
                ("inv_prop", C.c_double),
                ("inv_cols_count", C.c_ulong), ("inv_cols", C.POINTER(C.c_ulong)),
                ("freqs", c_double_p), ("subst_rates", c_double_p)]


MSA_STATS_DUP_TAXA, MSA_STATS_DUP_SEQS, MSA_STATS_GAP_PROP, MSA_STATS_GAP_SEQS, MSA_STATS_GAP_COLS = 1, 2, 4, 8, 16
MSA_STATS_INV_PROP, MSA_STATS_INV_COLS, MSA_STATS_FREQS, MSA_STATS_SUBST_RATES = 32, 64, 128, 256
MSA_STATS_ALL = (1 << (8 * C.sizeof(C.c_ulong))) - 1

TRAVERSE_CB = C.CFUNCTYPE(C.c_int, C.POINTER(UNode))
REDUCE_CB = C.CFUNCTYPE(None, C.c_void_p, c_double_p, C.c_size_t, C.c_int)

# every function the headers declare with PLL_EXPORT, for the symbol test
PLL_H_FUNCTIONS = """pll_partition_create pll_partition_destroy pll_set_tip_states
pll_set_tip_clv pll_set_pattern_weights pll_set_asc_bias_type pll_set_asc_state_weights
pll_set_subst_params pll_set_frequencies pll_set_category_rates pll_set_category_weights
pll_update_eigen pll_count_invariant_sites pll_update_invariant_sites
pll_update_invariant_sites_proportion pll_compute_gamma_cats pll_aligned_alloc
pll_aligned_free pll_get_sites_number pll_get_clv_size pll_update_prob_matrices
pll_update_partials pll_compute_root_loglikelihood pll_compute_edge_loglikelihood
pll_update_sumtable pll_compute_likelihood_derivatives pll_compute_node_ancestral
pll_show_pmatrix pll_show_clv pll_utree_traverse pll_utree_create_operations
pll_utree_wraptree pll_utree_wraptree_multi pll_utree_destroy pll_utree_graph_clone
pll_utree_graph_destroy pll_utree_clone pll_utree_reset_template_indices
pll_utree_check_integrity pll_utree_every pll_utree_parse_newick
pll_utree_parse_newick_unroot pll_utree_parse_newick_string
pll_utree_parse_newick_string_unroot pll_utree_export_newick pll_utree_show_ascii
pll_random_create pll_random_getint pll_random_destroy
pll_fasta_open pll_fasta_getnext pll_fasta_close pll_fasta_rewind pll_phylip_load pll_msa_destroy
pll_compress_site_patterns pll_compress_site_patterns_msa""".split()

PLLHIP_EVAL_H_FUNCTIONS = """pllhip_eval_create pllhip_eval_destroy pllhip_eval_set_partition
pllhip_eval_set_parallel_context pllhip_eval_set_root pllhip_eval_root pllhip_eval_invalidate_all
pllhip_eval_invalidate_pmatrix pllhip_eval_invalidate_clv pllhip_eval_loglh
pllhip_eval_set_branch_length pllhip_eval_optimize_branches pllhip_eval_ops
pllhip_eval_pmatrix_updates pllhip_eval_derivative_calls pllhip_eval_spr_round
pllhip_eval_set_fused pllhip_eval_newton_iterations pllhip_eval_set_brlen_linkage
pllhip_eval_set_brlen_scaler pllhip_eval_get_brlen_scaler pllhip_eval_get_partition_branch_length
pllhip_eval_set_partition_branch_length pllhip_eval_set_transient
pllhip_eval_site_rates pllhip_eval_destroy_site_rates pllhip_eval_optimize_rate_weights
pllhip_eval_rate_weights_trail
pllhip_substmap_counts pllhip_eval_substitution_map pllhip_eval_destroy_substitution_map
pllhip_eval_sample_ancestral pllhip_eval_destroy_sampled_ancestral
pllhip_history_rate_table pllhip_history_poisson pllhip_history_summary
pllhip_eval_sample_histories pllhip_eval_destroy_sampled_histories""".split()

PLLHIP_H_FUNCTIONS = """pllhip_device_count pllhip_set_device pllhip_get_device
pllhip_device_arch pllhip_eigen_decompose pllhip_sync_to_host pllhip_sync_to_device pllhip_get_clv
pllhip_get_scaler pllhip_get_sumtable pllhip_set_clv pllhip_set_scaler pllhip_synchronize
pllhip_stream pllhip_get_counters pllhip_reset_counters pllhip_partials_kernel_name
pllhip_comm_get_unique_id pllhip_comm_create pllhip_comm_destroy pllhip_reduce_cb
pllhip_profile_partials pllhip_profile_read pllhip_comm_rank pllhip_comm_size
pllhip_compute_likelihood_derivatives_multi pllhip_free_trial_lengths pllhip_set_sharding
pllhip_shard_count pllhip_results_create pllhip_results_destroy
pllhip_results_edge_loglikelihood pllhip_results_derivatives pllhip_results_fetch
pllhip_eval_attach_comm pllhip_update_partials_batch pllhip_results_poison pllhip_newton_branch pllhip_repeat_stats
pllhip_set_transient pllhip_discard_transient pllhip_transient_stats pllhip_newton_branch_multi
pllhip_schedule_stats pllhip_deferred_stats
pllhip_parsimony_tree_score pllhip_compress_last_times pllhip_compress_last_counts
pllhip_empirical_frequencies pllhip_empirical_subst_rates pllhip_empirical_invariant_sites
pllhip_msa_compute_stats pllhip_msa_destroy_stats pllhip_msa_stats_last_times
pllhip_treeset_create pllhip_treeset_destroy pllhip_treeset_count pllhip_treeset_add pllhip_treeset_splits
pllhip_treeset_rf_matrix pllhip_treeset_rf_to pllhip_treeset_support pllhip_treeset_last_sums pllhip_treeset_plan
pllhip_treeset_last_times pllhip_treeset_last_counts
pllhip_treeset_consensus pllhip_treeset_consensus_tree pllhip_treeset_tree_from_splits pllhip_consensus_needs
pllhip_treeset_last_consensus_counts
pllhip_node_ancestral_batch pllhip_node_ancestral_begin pllhip_node_ancestral_add pllhip_node_ancestral_finish
pllhip_node_ancestral_last_times
pllhip_sitelh_create pllhip_sitelh_destroy pllhip_sitelh_count pllhip_sitelh_get pllhip_sitelh_add
pllhip_sitelh_add_edge pllhip_sitelh_rell pllhip_rell_destroy pllhip_rell_last_times
pllhip_bootstrap_weights
pllhip_sitelh_au pllhip_au_destroy pllhip_au_last_times pllhip_multiscale_weights
pllhip_distances_partition pllhip_distances_msa pllhip_distmat_from_host pllhip_distmat_destroy pllhip_distmat_size
pllhip_distmat_get pllhip_distmat_compared pllhip_distmat_counts pllhip_distmat_no_overlap pllhip_distmat_nj
pllhip_distmat_nj_joins pllhip_distances_last_times
pllhip_simulate_edges pllhip_simulate_utree pllhip_simulate_last_times
pllhip_sitecat_edge pllhip_sitecat_from_table pllhip_sitecat_destroy pllhip_sitecat_sites pllhip_sitecat_categories
pllhip_sitecat_table pllhip_sitecat_posteriors pllhip_site_posteriors_destroy pllhip_sitecat_em_weights
pllhip_sitecat_last_times
pllhip_substmap_edge pllhip_edge_pairs_destroy pllhip_substmap_last_times
pllhip_sample_ancestral_edges pllhip_sample_ancestral_utree pllhip_ancsample_last_times
pllhip_sample_histories_edges pllhip_sample_histories_utree pllhip_history_last_times""".split()


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]
_libc.free.restype = None


def _libc_free(ptr):
    """free() of memory the library malloc()ed for its caller"""
    _libc.free(C.cast(ptr, C.c_void_p))


class CompressResult:
    """outcome of PllLib.compress_site_patterns: ok, errno, errmsg, length, rows (bytes per taxon), weights (uint32),
    site_pattern_map (uint32 per original site; the _msa form only), probe_steps / compares (pllhip_compress_last_counts)"""
    ok, errno, errmsg, length, rows, weights, site_pattern_map = False, 0, "", 0, None, None, None
    probe_steps, compares = 0, 0


PLLHIP_ANC_PROBS = 1


class AncestralResult(C.Structure):
    """pllhip_ancestral_t (include/pllhip_eval.h)"""
    _fields_ = [("node_count", C.c_uint), ("partition_count", C.c_uint),
                ("nodes", C.POINTER(C.c_void_p)), ("partition_indices", c_uint_p),
                ("site_offset", C.POINTER(C.c_size_t)), ("prob_offset", C.POINTER(C.c_size_t)),
                ("states", C.POINTER(C.POINTER(C.c_ubyte))), ("state_probs", C.POINTER(c_double_p)),
                ("probs", C.POINTER(c_double_p))]


class Ancestral:
    """numpy copy of a pllhip_ancestral_t: node_clv / node_index of the records in the reference's order,
    partition_indices, site_offset / prob_offset, states [node][sites] (uint8), state_probs [node][sites],
    probs [node][sum of sites x states] or None; rows(i, k) = the sites x states table of node i, local partition k"""

    def rows(self, i, k, states):
        a, b = self.prob_offset[k], self.prob_offset[k + 1]
        return self.probs[i, a:b].reshape(-1, states)


PLLHIP_SITECAT_POSTERIORS = 1
SITECAT_TRAIL_MAX = 64


class SitePosteriorsResult(C.Structure):
    """pllhip_site_posteriors_t (include/pllhip.h)"""
    _fields_ = [("sites", C.c_uint), ("cats", C.c_uint), ("rate", c_double_p), ("category", C.POINTER(C.c_ubyte)),
                ("category_prob", c_double_p), ("invariant_prob", c_double_p), ("lnl", c_double_p),
                ("posterior", c_double_p), ("expected", c_double_p), ("loglh", C.c_double)]


class SiteCatEmParams(C.Structure):
    """pllhip_sitecat_em_params_t"""
    _fields_ = [("start", c_double_p), ("epsilon", C.c_double), ("max_iterations", C.c_uint)]


class SitePosteriors:
    """numpy copy of a pllhip_site_posteriors_t: rate, category (uint8), category_prob, invariant_prob, lnl [sites]
    (rate / invariant_prob None for a set made from a host table), posterior [sites][cats] or None, expected [cats],
    loglh"""

    def __init__(self, res):
        n, r = res.sites, res.cats

        def take(ptr, shape, dtype=np.float64):
            return np.ctypeslib.as_array(ptr, shape=shape).astype(dtype, copy=True) if ptr and n else \
                (np.zeros(shape, dtype=dtype) if ptr else None)
        self.sites, self.cats, self.loglh = n, r, res.loglh
        self.rate, self.invariant_prob = take(res.rate, (n,)), take(res.invariant_prob, (n,))
        self.category = take(res.category, (n,), np.uint8)
        self.category_prob, self.lnl = take(res.category_prob, (n,)), take(res.lnl, (n,))
        self.posterior = take(res.posterior, (n, r))
        self.expected = np.ctypeslib.as_array(res.expected, shape=(r,)).copy()


PLLHIP_SUBST_SITES = 1


class EdgePairsResult(C.Structure):
    """pllhip_edge_pairs_t (include/pllhip.h)"""
    _fields_ = [("states", C.c_uint), ("cats", C.c_uint), ("sites", C.c_uint), ("F", c_double_p), ("pairs", c_double_p),
                ("posterior", c_double_p), ("differ", c_double_p), ("weight_sum", C.c_double),
                ("dropped", C.c_ulonglong)]


class BranchSubstResult(C.Structure):
    """pllhip_branch_subst_t (include/pllhip_eval.h)"""
    _fields_ = [("node", C.c_void_p), ("pairs", c_double_p), ("counts", c_double_p), ("dwell", c_double_p),
                ("differ", c_double_p), ("total", C.c_double), ("posterior_weight", C.c_double),
                ("dropped", C.c_ulonglong), ("states", C.c_uint), ("cats", C.c_uint), ("sites", C.c_uint)]


class SubstitutionMapResult(C.Structure):
    """pllhip_substitution_map_t"""
    _fields_ = [("partition_count", C.c_uint), ("branch_count", C.c_uint), ("partition_indices", c_uint_p),
                ("branches", C.POINTER(C.POINTER(BranchSubstResult)))]


class BranchSubst:
    """numpy copy of a pllhip_branch_subst_t: parent / child (clv indices of node and node->back), matrix, pairs
    [cats][S][S], counts [S][S], dwell [S], differ [sites] or None, total, posterior_weight, dropped"""


class EmFit:
    """outcome of an EM fit of the category weights: weights [cats], loglh, iterations (updates made), and the trail:
    trail_weights [evaluations][cats], trail_loglh [evaluations] (the first 64)"""


PLLHIP_RELL_REPLICATES = 1


class RellParams(C.Structure):
    """pllhip_rell_params_t"""
    _fields_ = [("replicates", C.c_uint), ("seed", C.c_ulonglong), ("flags", C.c_uint), ("batch", C.c_uint)]


class RellResult(C.Structure):
    """pllhip_rell_result_t"""
    _fields_ = [("trees", C.c_uint), ("replicates", C.c_uint), ("best", C.c_uint), ("batch", C.c_uint),
                ("lnl", c_double_p), ("bp_count", c_uint_p), ("kh_count", c_uint_p), ("sh_count", c_uint_p),
                ("elw", c_double_p), ("replicate_lnl", c_double_p)]


PLLHIP_AU_REPLICATES = 1


class AuParams(C.Structure):
    """pllhip_au_params_t"""
    _fields_ = [("replicates", C.c_uint), ("scales", C.c_uint), ("scale", c_double_p), ("seed", C.c_ulonglong),
                ("flags", C.c_uint), ("batch", C.c_uint)]


class AuResult(C.Structure):
    """pllhip_au_result_t"""
    _fields_ = [("trees", C.c_uint), ("replicates", C.c_uint), ("scales", C.c_uint), ("best", C.c_uint),
                ("batch", C.c_uint), ("lnl", c_double_p), ("draws", C.POINTER(C.c_ulonglong)), ("bp_count", c_uint_p),
                ("p_au", c_double_p), ("d", c_double_p), ("c", c_double_p), ("se", c_double_p), ("rss", c_double_p),
                ("used", c_uint_p), ("replicate_lnl", c_double_p)]


DIST_P, DIST_JC, DIST_ML = 0, 1, 2
DIST_KEEP_COUNTS = 1


class DistParams(C.Structure):
    """pllhip_dist_params_t"""
    _fields_ = [("method", C.c_int), ("flags", C.c_uint), ("min_dist", C.c_double), ("max_dist", C.c_double),
                ("budget_bytes", C.c_ulonglong), ("chunk_columns", C.c_uint)]


PLLHIP_SIM_INNER = 1


class SimParams(C.Structure):
    """pllhip_sim_params_t"""
    _fields_ = [("seed", C.c_ulonglong), ("first_site", C.c_ulonglong), ("sites", C.c_uint),
                ("first_replicate", C.c_uint), ("replicates", C.c_uint), ("flags", C.c_uint), ("alphabet", C.c_char_p)]


PLLHIP_ANCS_TIPS, PLLHIP_ANCS_COMPONENT = 1, 2


class AncSampleParams(C.Structure):
    """pllhip_ancsample_params_t, include/pllhip.h"""
    _fields_ = [("seed", C.c_ulonglong), ("first_replicate", C.c_uint), ("replicates", C.c_uint), ("flags", C.c_uint),
                ("alphabet", C.c_char_p)]


class SampledAncestralResult(C.Structure):
    """pllhip_sampled_ancestral_t, include/pllhip_eval.h"""
    _fields_ = [("partition_count", C.c_uint), ("node_count", C.c_uint), ("replicates", C.c_uint),
                ("partition_indices", C.POINTER(C.c_uint)), ("sites", C.POINTER(C.c_uint)),
                ("clv_index", C.POINTER(C.c_uint)), ("out", C.POINTER(C.POINTER(C.c_ubyte))),
                ("component", C.POINTER(C.POINTER(C.c_ubyte))), ("dropped", C.POINTER(C.c_ulonglong))]


class SampledAncestral:
    """one local partition of pllhip_eval_sample_ancestral: out uint8 [replicates][rows][sites], component
    [replicates][sites], dropped, clv_index [rows]"""


PLLHIP_HIST_SITES, PLLHIP_HIST_MAX_TABLE = 1 << 8, 1024


class SampledHistoriesResult(C.Structure):
    """pllhip_sampled_histories_t, include/pllhip_eval.h"""
    _fields_ = [("partition_count", C.c_uint), ("node_count", C.c_uint), ("replicates", C.c_uint),
                ("branch_count", C.c_uint), ("partition_indices", C.POINTER(C.c_uint)), ("sites", C.POINTER(C.c_uint)),
                ("states", C.POINTER(C.c_uint)), ("cats", C.POINTER(C.c_uint)), ("clv_index", C.POINTER(C.c_uint)),
                ("out", C.POINTER(C.POINTER(C.c_ubyte))), ("component", C.POINTER(C.POINTER(C.c_ubyte))),
                ("dropped", C.POINTER(C.c_ulonglong)), ("counts", C.POINTER(C.POINTER(C.c_ulonglong))),
                ("units", C.POINTER(C.POINTER(C.c_ulonglong))), ("dwell", C.POINTER(C.POINTER(C.c_double))),
                ("total", C.POINTER(C.POINTER(C.c_double))), ("dropped_edges", C.POINTER(C.POINTER(C.c_ulonglong))),
                ("changes", C.POINTER(C.POINTER(C.c_ubyte)))]


class SampledHistories:
    """one local partition of pllhip_eval_sample_histories, branches by pmatrix_index: out uint8
    [replicates][rows][sites], component [replicates][sites], dropped, clv_index [rows], counts uint64
    [replicates][branches][S][S], units uint64 [replicates][branches][R][S], dwell [replicates][branches][S], total
    [replicates][branches], dropped_edges uint64 [replicates][branches], changes uint8 [replicates][branches][sites] or
    None"""


class Rell:
    """numpy copy of a pllhip_rell_result_t: trees, replicates, best, batch, lnl, bp_count, kh_count, sh_count, elw,
    R [replicates][trees] or None, times = (draw, product, statistics) in ms"""


class Au:
    """numpy copy of a pllhip_au_result_t: trees, replicates, scales, best, batch, lnl [T], draws [K], bp_count [K][T],
    p_au / d / c / se / rss [T], used [T], R [scales][replicates][trees] or None, times = (draw, product, statistics)
    in ms"""


class PllLib:
    """One loaded implementation of include/pll.h."""

    def __init__(self, path=PRODUCT_LIB):
        if not os.path.exists(path):
            raise FileNotFoundError(
                f"{path} not found: build it first (python -c 'import __graft_entry__ as g; g.build()')")
        self.path = path
        self.lib = L = C.CDLL(path)
        self.is_product = hasattr(L, "pllhip_device_count")
        pp = C.POINTER(Partition)
        L.pll_partition_create.restype = pp
        L.pll_partition_create.argtypes = [C.c_uint] * 9
        L.pll_partition_destroy.argtypes = [pp]
        L.pll_get_sites_number.argtypes = [pp, C.c_uint]
        L.pll_get_sites_number.restype = C.c_uint
        L.pll_get_clv_size.argtypes = [pp, C.c_uint]
        L.pll_get_clv_size.restype = C.c_uint
        L.pll_set_tip_states.argtypes = [pp, C.c_uint, C.POINTER(C.c_ulonglong), C.c_char_p]
        L.pll_set_tip_clv.argtypes = [pp, C.c_uint, c_double_p, C.c_int]
        L.pll_set_pattern_weights.argtypes = [pp, c_uint_p]
        L.pll_set_asc_bias_type.argtypes = [pp, C.c_int]
        L.pll_set_asc_state_weights.argtypes = [pp, c_uint_p]
        L.pll_set_asc_state_weights.restype = None
        L.pll_set_subst_params.argtypes = [pp, C.c_uint, c_double_p]
        L.pll_set_frequencies.argtypes = [pp, C.c_uint, c_double_p]
        L.pll_set_category_rates.argtypes = [pp, c_double_p]
        L.pll_set_category_weights.argtypes = [pp, c_double_p]
        L.pll_update_eigen.argtypes = [pp, C.c_uint]
        L.pll_update_invariant_sites.argtypes = [pp]
        L.pll_update_invariant_sites_proportion.argtypes = [pp, C.c_uint, C.c_double]
        L.pll_count_invariant_sites.argtypes = [pp, c_uint_p]
        L.pll_count_invariant_sites.restype = C.c_uint
        L.pll_compute_gamma_cats.argtypes = [C.c_double, C.c_uint, c_double_p, C.c_int]
        L.pll_update_prob_matrices.argtypes = [pp, c_uint_p, c_uint_p, c_double_p, C.c_uint]
        L.pll_update_partials.argtypes = [pp, C.POINTER(Operation), C.c_uint]
        L.pll_update_partials.restype = None
        L.pll_compute_edge_loglikelihood.restype = C.c_double
        L.pll_compute_edge_loglikelihood.argtypes = [pp, C.c_uint, C.c_int, C.c_uint, C.c_int,
                                                     C.c_uint, c_uint_p, c_double_p]
        L.pll_compute_root_loglikelihood.restype = C.c_double
        L.pll_compute_root_loglikelihood.argtypes = [pp, C.c_uint, C.c_int, c_uint_p, c_double_p]
        L.pll_update_sumtable.argtypes = [pp, C.c_uint, C.c_uint, C.c_int, C.c_int, c_uint_p, c_double_p]
        L.pll_compute_likelihood_derivatives.argtypes = [pp, C.c_int, C.c_int, C.c_double, c_uint_p,
                                                         c_double_p, c_double_p, c_double_p]
        L.pll_compute_node_ancestral.argtypes = [pp, C.c_uint, C.c_int, C.c_uint, C.c_int, C.c_uint,
                                                 c_uint_p, c_double_p]
        L.pll_aligned_alloc.restype = C.c_void_p
        L.pll_aligned_alloc.argtypes = [C.c_size_t, C.c_size_t]
        L.pll_aligned_free.argtypes = [C.c_void_p]
        up, tp = C.POINTER(UNode), C.POINTER(UTree)
        L.pll_utree_parse_newick_string.restype = tp
        L.pll_utree_parse_newick_string.argtypes = [C.c_char_p]
        L.pll_utree_parse_newick_string_unroot.restype = tp
        L.pll_utree_parse_newick_string_unroot.argtypes = [C.c_char_p]
        L.pll_utree_destroy.argtypes = [tp, C.c_void_p]
        L.pll_utree_clone.restype = tp
        L.pll_utree_clone.argtypes = [tp]
        L.pll_utree_check_integrity.argtypes = [tp]
        L.pll_utree_traverse.argtypes = [up, C.c_int, TRAVERSE_CB, C.POINTER(up), c_uint_p]
        L.pll_utree_create_operations.restype = None
        L.pll_utree_create_operations.argtypes = [C.POINTER(up), C.c_uint, c_double_p, c_uint_p,
                                                  C.POINTER(Operation), c_uint_p, c_uint_p]
        L.pll_utree_export_newick.restype = C.c_void_p
        L.pll_utree_export_newick.argtypes = [up, C.c_void_p]
        L.pll_fastparsimony_init.restype = C.c_void_p
        L.pll_fastparsimony_init.argtypes = [pp]
        L.pll_parsimony_destroy.restype = None
        L.pll_parsimony_destroy.argtypes = [C.c_void_p]
        L.pll_fastparsimony_stepwise.restype = tp
        L.pll_fastparsimony_stepwise.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_char_p), c_uint_p,
                                                 C.c_uint, C.c_uint]
        L.pll_fastparsimony_stepwise_extend.argtypes = [tp, C.POINTER(C.c_void_p), C.c_uint, C.POINTER(C.c_char_p),
                                                        c_uint_p, C.c_uint, c_uint_p]
        L.pll_fastparsimony_stepwise_spr_round.argtypes = [tp, C.POINTER(C.c_void_p), C.c_uint, c_uint_p, C.c_uint,
                                                           C.POINTER(C.c_int), c_uint_p]
        mp = C.POINTER(Msa)
        L.pll_fasta_open.restype = C.c_void_p
        L.pll_fasta_open.argtypes = [C.c_char_p, c_uint_p]
        L.pll_fasta_getnext.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_long), C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_long), C.POINTER(C.c_long)]
        L.pll_fasta_close.restype = None
        L.pll_fasta_close.argtypes = [C.c_void_p]
        L.pll_fasta_rewind.argtypes = [C.c_void_p]
        L.pll_phylip_load.restype = mp
        L.pll_phylip_load.argtypes = [C.c_char_p, C.c_int]
        L.pll_msa_destroy.restype = None
        L.pll_msa_destroy.argtypes = [mp]
        L.pll_compress_site_patterns.restype = c_uint_p
        L.pll_compress_site_patterns.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_ulonglong), C.c_int,
                                                 C.POINTER(C.c_int)]
        L.pll_compress_site_patterns_msa.restype = c_uint_p
        L.pll_compress_site_patterns_msa.argtypes = [mp, C.POINTER(C.c_ulonglong), c_uint_p]
        if hasattr(L, "pllhip_eval_create"):
            L.pllhip_eval_create.restype = C.c_void_p
            L.pllhip_eval_create.argtypes = [tp, C.c_uint, C.c_uint]
            L.pllhip_eval_destroy.argtypes = [C.c_void_p]
            L.pllhip_eval_set_partition.argtypes = [C.c_void_p, C.c_uint, pp, c_uint_p]
            L.pllhip_eval_set_parallel_context.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            L.pllhip_eval_set_root.argtypes = [C.c_void_p, up]
            L.pllhip_eval_root.restype = up
            L.pllhip_eval_root.argtypes = [C.c_void_p]
            L.pllhip_eval_invalidate_all.argtypes = [C.c_void_p]
            L.pllhip_eval_invalidate_pmatrix.argtypes = [C.c_void_p, up]
            L.pllhip_eval_invalidate_clv.argtypes = [C.c_void_p, up]
            L.pllhip_eval_loglh.restype = C.c_double
            L.pllhip_eval_loglh.argtypes = [C.c_void_p, C.c_int]
            L.pllhip_eval_set_branch_length.argtypes = [C.c_void_p, up, C.c_double]
            L.pllhip_eval_set_transient.argtypes = [C.c_void_p, C.c_int]
            L.pllhip_eval_set_transient.restype = None
            L.pllhip_eval_optimize_branches.restype = C.c_double
            L.pllhip_eval_optimize_branches.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double,
                                                        C.c_int, C.c_int]
            L.pllhip_eval_set_brlen_linkage.argtypes = [C.c_void_p, C.c_int]
            L.pllhip_eval_set_brlen_scaler.argtypes = [C.c_void_p, C.c_uint, C.c_double]
            L.pllhip_eval_get_brlen_scaler.restype = C.c_double
            L.pllhip_eval_get_brlen_scaler.argtypes = [C.c_void_p, C.c_uint]
            L.pllhip_eval_get_partition_branch_length.restype = C.c_double
            L.pllhip_eval_get_partition_branch_length.argtypes = [C.c_void_p, C.c_uint, up]
            L.pllhip_eval_set_partition_branch_length.argtypes = [C.c_void_p, C.c_uint, up, C.c_double]
            L.pllhip_eval_spr_round.restype = C.c_double
            L.pllhip_eval_spr_round.argtypes = [C.c_void_p, C.POINTER(SprParams), C.POINTER(SprCutoff),
                                                C.POINTER(SprStats)]
            if hasattr(L, "pllhip_eval_compute_ancestral"):
                L.pllhip_eval_compute_ancestral.restype = C.POINTER(AncestralResult)
                L.pllhip_eval_compute_ancestral.argtypes = [C.c_void_p, C.c_uint]
                L.pllhip_eval_destroy_ancestral.restype = None
                L.pllhip_eval_destroy_ancestral.argtypes = [C.POINTER(AncestralResult)]
            if hasattr(L, "pllhip_eval_site_rates"):
                L.pllhip_eval_site_rates.restype = C.POINTER(C.POINTER(SitePosteriorsResult))
                L.pllhip_eval_site_rates.argtypes = [C.c_void_p, C.c_uint]
                L.pllhip_eval_destroy_site_rates.restype = None
                L.pllhip_eval_destroy_site_rates.argtypes = [C.POINTER(C.POINTER(SitePosteriorsResult))]
                L.pllhip_eval_optimize_rate_weights.restype = C.c_double
                L.pllhip_eval_optimize_rate_weights.argtypes = [C.c_void_p, C.c_uint, C.c_double, C.c_uint]
                L.pllhip_eval_rate_weights_trail.restype = C.c_uint
                L.pllhip_eval_rate_weights_trail.argtypes = [C.c_void_p, c_double_p, c_double_p]
            if hasattr(L, "pllhip_eval_sample_ancestral"):
                L.pllhip_eval_sample_ancestral.restype = C.POINTER(SampledAncestralResult)
                L.pllhip_eval_sample_ancestral.argtypes = [C.c_void_p, C.POINTER(AncSampleParams)]
                L.pllhip_eval_destroy_sampled_ancestral.restype = None
                L.pllhip_eval_destroy_sampled_ancestral.argtypes = [C.POINTER(SampledAncestralResult)]
            if hasattr(L, "pllhip_eval_sample_histories"):
                ull_p = C.POINTER(C.c_ulonglong)
                L.pllhip_history_rate_table.argtypes = [C.c_uint, C.c_uint, c_double_p, c_double_p, c_double_p, C.c_uint,
                                                        c_double_p, c_double_p]
                L.pllhip_history_poisson.argtypes = [C.c_double, c_double_p, c_uint_p]
                L.pllhip_history_summary.argtypes = [C.c_uint, C.c_uint, c_double_p, ull_p, ull_p, c_double_p, c_double_p,
                                                     c_double_p]
                L.pllhip_eval_sample_histories.restype = C.POINTER(SampledHistoriesResult)
                L.pllhip_eval_sample_histories.argtypes = [C.c_void_p, C.POINTER(AncSampleParams)]
                L.pllhip_eval_destroy_sampled_histories.restype = None
                L.pllhip_eval_destroy_sampled_histories.argtypes = [C.POINTER(SampledHistoriesResult)]
            if hasattr(L, "pllhip_eval_substitution_map"):
                L.pllhip_substmap_counts.argtypes = [C.c_uint, C.c_uint, c_double_p, c_double_p, c_double_p, C.c_double,
                                                     c_double_p, c_double_p, c_double_p]
                L.pllhip_eval_substitution_map.restype = C.POINTER(SubstitutionMapResult)
                L.pllhip_eval_substitution_map.argtypes = [C.c_void_p, C.c_uint]
                L.pllhip_eval_destroy_substitution_map.restype = None
                L.pllhip_eval_destroy_substitution_map.argtypes = [C.POINTER(SubstitutionMapResult)]
            for fn in ("pllhip_eval_ops", "pllhip_eval_pmatrix_updates", "pllhip_eval_derivative_calls",
                       "pllhip_eval_newton_iterations"):
                getattr(L, fn).restype = C.c_ulong
                getattr(L, fn).argtypes = [C.c_void_p]
        if self.is_product:
            L.pllhip_device_count.restype = C.c_int
            L.pllhip_set_device.argtypes = [C.c_int]
            L.pllhip_device_arch.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
            L.pllhip_eigen_decompose.argtypes = [C.c_uint, C.c_uint, c_double_p, c_double_p,
                                                 c_double_p, c_double_p, c_double_p]
            L.pllhip_sync_to_host.argtypes = [pp, C.c_uint]
            L.pllhip_sync_to_device.argtypes = [pp, C.c_uint]
            L.pllhip_get_clv.argtypes = [pp, C.c_uint, c_double_p]
            L.pllhip_set_clv.argtypes = [pp, C.c_uint, c_double_p]
            L.pllhip_get_scaler.argtypes = [pp, C.c_uint, c_uint_p]
            L.pllhip_set_scaler.argtypes = [pp, C.c_uint, c_uint_p]
            L.pllhip_get_sumtable.argtypes = [pp, c_double_p, c_double_p]
            L.pllhip_synchronize.argtypes = [pp]
            L.pllhip_stream.restype = C.c_void_p
            L.pllhip_stream.argtypes = [pp]
            L.pllhip_get_counters.argtypes = [pp, C.POINTER(Counters)]
            L.pllhip_reset_counters.argtypes = [pp]
            L.pllhip_partials_kernel_name.restype = C.c_char_p
            L.pllhip_partials_kernel_name.argtypes = [pp]
            L.pllhip_profile_partials.argtypes = [pp, C.c_int]
            L.pllhip_profile_read.argtypes = [pp, C.POINTER(Profile)]
            L.pllhip_repeat_stats.argtypes = [pp, C.POINTER(RepeatStats)]
            L.pllhip_set_transient.argtypes = [pp, C.c_int]
            L.pllhip_discard_transient.argtypes = [pp]
            L.pllhip_transient_stats.argtypes = [pp, C.POINTER(TransientStats)]
            L.pllhip_schedule_stats.argtypes = [pp, C.POINTER(ScheduleStats)]
            L.pllhip_deferred_stats.argtypes = [pp, C.POINTER(DeferredStats)]
            L.pllhip_comm_get_unique_id.argtypes = [C.c_char_p]
            L.pllhip_comm_create.restype = C.c_void_p
            L.pllhip_comm_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int]
            L.pllhip_comm_destroy.argtypes = [C.c_void_p]
            L.pllhip_reduce_cb.restype = None
            L.pllhip_reduce_cb.argtypes = [C.c_void_p, c_double_p, C.c_size_t, C.c_int]
            L.pllhip_set_sharding.argtypes = [C.c_uint, C.POINTER(C.c_int)]
            L.pllhip_shard_count.argtypes = [pp]
            L.pllhip_shard_count.restype = C.c_uint
            L.pllhip_parsimony_tree_score.argtypes = [C.POINTER(C.c_void_p), C.c_uint, tp, c_uint_p]
            L.pllhip_compress_last_times.restype = None
            L.pllhip_compress_last_times.argtypes = [c_double_p, c_double_p, c_double_p]
            L.pllhip_compress_last_counts.restype = None
            L.pllhip_compress_last_counts.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
            L.pllhip_comm_rank.argtypes = [C.c_void_p]
            L.pllhip_comm_size.argtypes = [C.c_void_p]
            L.pllhip_eval_attach_comm.argtypes = [C.c_void_p, C.c_void_p]
            L.pllhip_eval_set_fused.argtypes = [C.c_void_p, C.c_void_p]
            L.pllhip_eval_set_fused.restype = None
            L.pllhip_results_create.restype = C.c_void_p
            L.pllhip_results_create.argtypes = [C.c_void_p, C.c_uint]
            L.pllhip_results_destroy.argtypes = [C.c_void_p]
            L.pllhip_results_edge_loglikelihood.argtypes = [C.c_void_p, C.c_uint, pp, C.c_uint, C.c_int,
                                                            C.c_uint, C.c_int, C.c_uint, c_uint_p]
            L.pllhip_results_derivatives.argtypes = [C.c_void_p, C.c_uint, pp, C.c_int, C.c_int, c_double_p,
                                                     C.c_uint, c_uint_p, c_double_p]
            L.pllhip_results_fetch.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_int, c_double_p]
            L.pllhip_results_poison.argtypes = [C.c_void_p]
            L.pllhip_results_poison.restype = None
        if hasattr(L, "pllhip_node_ancestral_batch"):
            L.pllhip_node_ancestral_batch.argtypes = [pp, C.c_uint, c_uint_p, c_uint_p, c_uint_p, c_uint_p, C.c_uint,
                                                      C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                      C.POINTER(C.c_void_p)]
            L.pllhip_node_ancestral_begin.restype = C.c_void_p
            L.pllhip_node_ancestral_begin.argtypes = [pp, C.c_uint, C.c_uint]
            L.pllhip_node_ancestral_add.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, c_uint_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p]
            L.pllhip_node_ancestral_finish.argtypes = [C.c_void_p]
            L.pllhip_node_ancestral_last_times.restype = None
            L.pllhip_node_ancestral_last_times.argtypes = [c_double_p, C.POINTER(C.c_ulonglong)]
        if hasattr(L, "pllhip_sitecat_edge"):
            sp = C.POINTER(SitePosteriorsResult)
            L.pllhip_sitecat_edge.restype = C.c_void_p
            L.pllhip_sitecat_edge.argtypes = [pp, C.c_uint, C.c_int, C.c_uint, C.c_int, C.c_uint, c_uint_p]
            L.pllhip_sitecat_from_table.restype = C.c_void_p
            L.pllhip_sitecat_from_table.argtypes = [C.c_uint, C.c_uint, c_double_p, c_uint_p, c_double_p]
            L.pllhip_sitecat_destroy.restype = None
            L.pllhip_sitecat_destroy.argtypes = [C.c_void_p]
            L.pllhip_sitecat_sites.restype = C.c_uint
            L.pllhip_sitecat_sites.argtypes = [C.c_void_p]
            L.pllhip_sitecat_categories.restype = C.c_uint
            L.pllhip_sitecat_categories.argtypes = [C.c_void_p]
            L.pllhip_sitecat_table.argtypes = [C.c_void_p, c_double_p, c_double_p, c_uint_p]
            L.pllhip_sitecat_posteriors.restype = sp
            L.pllhip_sitecat_posteriors.argtypes = [C.c_void_p, c_double_p, C.c_uint]
            L.pllhip_site_posteriors_destroy.restype = None
            L.pllhip_site_posteriors_destroy.argtypes = [sp]
            L.pllhip_sitecat_em_weights.argtypes = [C.c_void_p, C.POINTER(SiteCatEmParams), c_double_p, c_double_p,
                                                    c_uint_p, c_double_p, c_double_p]
            L.pllhip_sitecat_last_times.restype = None
            L.pllhip_sitecat_last_times.argtypes = [c_double_p, c_double_p, c_double_p]
        if hasattr(L, "pllhip_substmap_edge"):
            L.pllhip_substmap_edge.restype = C.POINTER(EdgePairsResult)
            L.pllhip_substmap_edge.argtypes = [pp, C.c_uint, C.c_int, C.c_uint, C.c_int, C.c_uint, c_uint_p, C.c_uint]
            L.pllhip_edge_pairs_destroy.restype = None
            L.pllhip_edge_pairs_destroy.argtypes = [C.POINTER(EdgePairsResult)]
            L.pllhip_substmap_last_times.restype = None
            L.pllhip_substmap_last_times.argtypes = [c_double_p, c_double_p, c_double_p]
        if hasattr(L, "pllhip_sitelh_rell"):
            L.pllhip_sitelh_create.restype = C.c_void_p
            L.pllhip_sitelh_create.argtypes = [C.c_uint, c_uint_p]
            L.pllhip_sitelh_destroy.restype = None
            L.pllhip_sitelh_destroy.argtypes = [C.c_void_p]
            L.pllhip_sitelh_count.restype = C.c_uint
            L.pllhip_sitelh_count.argtypes = [C.c_void_p]
            L.pllhip_sitelh_get.argtypes = [C.c_void_p, C.c_uint, c_double_p]
            L.pllhip_sitelh_add.argtypes = [C.c_void_p, c_double_p]
            L.pllhip_sitelh_add_edge.argtypes = [C.c_void_p, C.c_uint, C.c_uint, pp, C.c_uint, C.c_int, C.c_uint,
                                                 C.c_int, C.c_uint, c_uint_p, c_double_p]
            L.pllhip_sitelh_rell.restype = C.POINTER(RellResult)
            L.pllhip_sitelh_rell.argtypes = [C.c_void_p, C.POINTER(RellParams)]
            L.pllhip_rell_destroy.restype = None
            L.pllhip_rell_destroy.argtypes = [C.POINTER(RellResult)]
            L.pllhip_rell_last_times.restype = None
            L.pllhip_rell_last_times.argtypes = [c_double_p, c_double_p, c_double_p]
            L.pllhip_bootstrap_weights.argtypes = [c_uint_p, C.c_uint, C.c_ulonglong, C.c_uint, C.c_uint, c_uint_p]
        if hasattr(L, "pllhip_sitelh_au"):
            L.pllhip_sitelh_au.restype = C.POINTER(AuResult)
            L.pllhip_sitelh_au.argtypes = [C.c_void_p, C.POINTER(AuParams)]
            L.pllhip_au_destroy.restype = None
            L.pllhip_au_destroy.argtypes = [C.POINTER(AuResult)]
            L.pllhip_au_last_times.restype = None
            L.pllhip_au_last_times.argtypes = [c_double_p, c_double_p, c_double_p]
            L.pllhip_multiscale_weights.argtypes = [c_uint_p, C.c_uint, C.c_ulonglong, C.c_uint, C.c_ulonglong,
                                                    C.c_uint, C.c_uint, c_uint_p]
        if hasattr(L, "pllhip_distances_partition"):
            L.pllhip_distances_partition.restype = C.c_void_p
            L.pllhip_distances_partition.argtypes = [pp, C.POINTER(DistParams)]
            L.pllhip_distances_msa.restype = C.c_void_p
            L.pllhip_distances_msa.argtypes = [mp, C.c_uint, C.POINTER(C.c_ulonglong), c_uint_p, C.POINTER(DistParams)]
            L.pllhip_distmat_from_host.restype = C.c_void_p
            L.pllhip_distmat_from_host.argtypes = [C.c_uint, c_double_p]
            L.pllhip_distmat_destroy.restype = None
            L.pllhip_distmat_destroy.argtypes = [C.c_void_p]
            L.pllhip_distmat_size.restype = C.c_uint
            L.pllhip_distmat_size.argtypes = [C.c_void_p]
            L.pllhip_distmat_get.argtypes = [C.c_void_p, c_double_p]
            L.pllhip_distmat_compared.argtypes = [C.c_void_p, c_uint_p]
            L.pllhip_distmat_counts.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.POINTER(C.c_int)]
            L.pllhip_distmat_no_overlap.restype = C.c_ulonglong
            L.pllhip_distmat_no_overlap.argtypes = [C.c_void_p]
            L.pllhip_distmat_nj.restype = tp
            L.pllhip_distmat_nj.argtypes = [C.c_void_p, C.POINTER(C.c_char_p)]
            L.pllhip_distmat_nj_joins.argtypes = [C.c_void_p, c_uint_p, c_double_p]
            L.pllhip_distances_last_times.restype = None
            L.pllhip_distances_last_times.argtypes = [c_double_p] * 5
        if hasattr(L, "pllhip_simulate_edges"):
            ubyte_p = C.POINTER(C.c_ubyte)
            L.pllhip_simulate_edges.argtypes = [pp, C.POINTER(SimParams), C.c_uint, C.c_uint, c_uint_p, c_uint_p, c_uint_p,
                                                c_uint_p, C.c_uint, ubyte_p]
            L.pllhip_simulate_utree.argtypes = [pp, C.POINTER(SimParams), up, c_uint_p, C.c_int, ubyte_p]
            L.pllhip_simulate_last_times.restype = None
            L.pllhip_simulate_last_times.argtypes = [c_double_p, c_double_p, c_double_p, C.POINTER(C.c_ulonglong)]
        if hasattr(L, "pllhip_sample_ancestral_edges"):
            ubyte_p, ull_p = C.POINTER(C.c_ubyte), C.POINTER(C.c_ulonglong)
            L.pllhip_sample_ancestral_edges.argtypes = [pp, C.POINTER(AncSampleParams), C.c_uint, C.c_int, C.c_uint, C.c_int,
                                                        C.c_uint, c_uint_p, c_uint_p, c_uint_p, c_uint_p, C.c_uint,
                                                        ubyte_p, ubyte_p, ull_p]
            L.pllhip_sample_ancestral_utree.argtypes = [pp, C.POINTER(AncSampleParams), up, c_uint_p, ubyte_p, ubyte_p, ull_p]
            L.pllhip_ancsample_last_times.restype = None
            L.pllhip_ancsample_last_times.argtypes = [c_double_p, c_double_p, c_double_p, ull_p]
        if hasattr(L, "pllhip_sample_histories_edges"):
            ubyte_p, ull_p = C.POINTER(C.c_ubyte), C.POINTER(C.c_ulonglong)
            L.pllhip_sample_histories_edges.argtypes = [pp, C.POINTER(AncSampleParams), C.c_uint, C.c_int, C.c_uint, C.c_int,
                                                        C.c_uint, c_uint_p, c_uint_p, c_uint_p, c_uint_p, C.c_uint,
                                                        c_uint_p, c_double_p, ubyte_p, ubyte_p, ull_p, ull_p, ull_p,
                                                        ubyte_p, ull_p]
            L.pllhip_sample_histories_utree.argtypes = [pp, C.POINTER(AncSampleParams), up, c_uint_p, c_uint_p, ubyte_p,
                                                        ubyte_p, ull_p, ull_p, ull_p, ubyte_p, ull_p, c_uint_p, c_uint_p]
            L.pllhip_history_last_times.restype = None
            L.pllhip_history_last_times.argtypes = [c_double_p, c_double_p, c_double_p, c_double_p]
        if hasattr(L, "pllhip_msa_compute_stats"):
            L.pllhip_empirical_frequencies.restype = c_double_p
            L.pllhip_empirical_frequencies.argtypes = [pp]
            L.pllhip_empirical_subst_rates.restype = c_double_p
            L.pllhip_empirical_subst_rates.argtypes = [pp]
            L.pllhip_empirical_invariant_sites.restype = C.c_double
            L.pllhip_empirical_invariant_sites.argtypes = [pp]
            L.pllhip_msa_compute_stats.restype = C.POINTER(MsaStats)
            L.pllhip_msa_compute_stats.argtypes = [mp, C.c_uint, C.POINTER(C.c_ulonglong), c_uint_p, C.c_ulong]
            L.pllhip_msa_destroy_stats.restype = None
            L.pllhip_msa_destroy_stats.argtypes = [C.POINTER(MsaStats)]
            L.pllhip_msa_stats_last_times.restype = None
            L.pllhip_msa_stats_last_times.argtypes = [c_double_p, c_double_p]
        if hasattr(L, "pllhip_treeset_create"):
            ull_p = C.POINTER(C.c_ulonglong)
            L.pllhip_treeset_create.restype = C.c_void_p
            L.pllhip_treeset_create.argtypes = [C.c_uint, C.POINTER(C.c_char_p)]
            L.pllhip_treeset_destroy.restype = None
            L.pllhip_treeset_destroy.argtypes = [C.c_void_p]
            L.pllhip_treeset_count.restype = C.c_uint
            L.pllhip_treeset_count.argtypes = [C.c_void_p]
            L.pllhip_treeset_add.argtypes = [C.c_void_p, tp]
            L.pllhip_treeset_splits.argtypes = [C.c_void_p, C.c_uint, c_uint_p]
            L.pllhip_treeset_rf_matrix.argtypes = [C.c_void_p, c_uint_p]
            L.pllhip_treeset_rf_to.argtypes = [C.c_void_p, tp, c_uint_p]
            L.pllhip_treeset_support.argtypes = [C.c_void_p, tp, C.c_int, c_double_p, C.POINTER(up)]
            L.pllhip_treeset_last_sums.restype = C.c_uint
            L.pllhip_treeset_last_sums.argtypes = [ull_p, C.c_uint]
            L.pllhip_treeset_plan.argtypes = [C.c_void_p, C.c_uint, c_uint_p, c_uint_p, c_uint_p, c_uint_p, c_uint_p]
            L.pllhip_treeset_last_times.restype = None
            L.pllhip_treeset_last_times.argtypes = [c_double_p, c_double_p, c_double_p]
            L.pllhip_treeset_last_counts.restype = None
            L.pllhip_treeset_last_counts.argtypes = [ull_p, ull_p]
        if hasattr(L, "pllhip_treeset_consensus"):
            ull_p = C.POINTER(C.c_ulonglong)
            L.pllhip_treeset_consensus.argtypes = [C.c_void_p, C.c_double, c_uint_p, c_uint_p, c_uint_p, c_double_p]
            L.pllhip_treeset_consensus_tree.restype = tp
            L.pllhip_treeset_consensus_tree.argtypes = [C.c_void_p, C.c_double]
            L.pllhip_treeset_tree_from_splits.restype = tp
            L.pllhip_treeset_tree_from_splits.argtypes = [C.c_void_p, C.c_uint, c_uint_p, c_double_p]
            L.pllhip_consensus_needs.argtypes = [C.c_uint, C.c_double, c_uint_p, c_uint_p]
            L.pllhip_treeset_last_consensus_counts.restype = None
            L.pllhip_treeset_last_consensus_counts.argtypes = [ull_p, ull_p]
        if hasattr(L, "pllhip_newton_branch"):
            L.pllhip_newton_branch.argtypes = [pp, C.c_int, C.c_int, c_uint_p, c_double_p, C.c_double, C.c_double,
                                               C.c_double, C.c_double, C.c_uint, c_double_p, c_uint_p, c_double_p]
        if hasattr(L, "pllhip_newton_branch_multi"):
            L.pllhip_newton_branch_multi.argtypes = [C.POINTER(pp), C.c_uint, C.c_int, C.c_int, C.POINTER(c_uint_p),
                                                     C.POINTER(c_double_p), c_double_p, C.c_double, C.c_double, C.c_double,
                                                     C.c_double, C.c_uint, c_double_p, c_uint_p, c_double_p]
        if hasattr(L, "pllhip_update_partials_batch"):
            L.pllhip_update_partials_batch.argtypes = [C.POINTER(pp), C.c_uint, C.POINTER(Operation), C.c_uint]
        if hasattr(L, "pllhip_compute_likelihood_derivatives_multi"):
            L.pllhip_compute_likelihood_derivatives_multi.argtypes = [pp, C.c_int, C.c_int, c_double_p, C.c_uint,
                                                                      c_uint_p, c_double_p, c_double_p, c_double_p]

    # --- error state ------------------------------------------------------
    @property
    def errno(self):
        return C.c_int.in_dll(self.lib, "pll_errno").value

    @errno.setter
    def errno(self, v):
        C.c_int.in_dll(self.lib, "pll_errno").value = v

    @property
    def errmsg(self):
        return (C.c_char * 200).in_dll(self.lib, "pll_errmsg").value.decode(errors="replace")

    # --- alignment input ----------------------------------------------------
    def char_map(self, name):
        """pll_map_nt / pll_map_aa / pll_map_bin (256 pll_state_t) or pll_map_fasta (256 unsigned) of the library"""
        ctype = C.c_uint if name == "pll_map_fasta" else C.c_ulonglong
        return (ctype * 256).in_dll(self.lib, name)

    def fasta_open(self, path, status=None):
        """pll_fasta_t * (or None, see errno); status: 256 unsigned, default pll_map_fasta"""
        status = self.char_map("pll_map_fasta") if status is None else (C.c_uint * 256)(*[int(x) for x in status])
        self._fasta_status = status                                   # the handle keeps the pointer
        return self.lib.pll_fasta_open(os.fsencode(str(path)), status)

    def fasta_getnext(self, fd):
        """(head, head_len, seq, seq_len, seqno) with head / seq as bytes, or None (see errno)"""
        head, seq = C.c_void_p(), C.c_void_p()
        hl, sl, no = C.c_long(-1), C.c_long(-1), C.c_long(-1)
        if not self.lib.pll_fasta_getnext(fd, C.byref(head), C.byref(hl), C.byref(seq), C.byref(sl), C.byref(no)):
            return None
        out = (C.string_at(head.value), hl.value, C.string_at(seq.value), sl.value, no.value)
        _libc_free(head)
        _libc_free(seq)
        return out

    def phylip_load(self, path, interleaved=False):
        """pll_msa_t * (a ctypes pointer; falsy on failure, see errno); free it with lib.pll_msa_destroy"""
        return self.lib.pll_phylip_load(os.fsencode(str(path)), 1 if interleaved else 0)

    @staticmethod
    def msa_contents(msa):
        """(count, length, labels, sequences) of a pll_msa_t *, strings as bytes up to their NUL"""
        m = msa.contents
        return (m.count, m.length, [m.label[i] for i in range(m.count)],
                [C.string_at(m.sequence[i]) for i in range(m.count)])

    def compress_site_patterns(self, rows, charmap, count=None, length=None, msa_form=False, want_map=True):
        """pll_compress_site_patterns (msa_form: pll_compress_site_patterns_msa) on a copy of `rows` ([T][L] bytes).
        Returns a CompressResult; .ok is False when the call returned NULL."""
        rows = [bytes(r) for r in rows]
        T = len(rows) if count is None else count
        L = (len(rows[0]) if rows else 0) if length is None else length
        bufs = [C.create_string_buffer(r, len(r) + 1) for r in rows]
        seqs = (C.c_void_p * max(1, len(bufs)))(*[C.addressof(b) for b in bufs])
        cmap = (C.c_ulonglong * 256)(*[int(x) for x in charmap])
        res = CompressResult()
        self.errno = 0
        if msa_form:
            msa = Msa(T, L, seqs, None)
            spm = np.full(max(L, 1), 0xffffffff, dtype=np.uint32)
            w = self.lib.pll_compress_site_patterns_msa(C.byref(msa), cmap, spm.ctypes.data_as(c_uint_p) if want_map else None)
            res.length = msa.length
            res.site_pattern_map = spm[:L] if want_map else None
        else:
            n = C.c_int(L)
            w = self.lib.pll_compress_site_patterns(seqs, cmap, T, C.byref(n))
            res.length = n.value
        res.ok = bool(w)
        res.errno, res.errmsg = self.errno, self.errmsg
        if res.ok:
            res.weights = np.ctypeslib.as_array(w, shape=(res.length,)).copy()
            _libc_free(w)
            res.rows = [C.string_at(C.addressof(b)) for b in bufs]     # up to the NUL the call wrote
            if self.is_product:
                res.probe_steps, res.compares = self.compress_last_counts()
        else:
            res.rows = [b.raw[:-1] for b in bufs]                      # the whole buffers: must be untouched
        return res

    def compress_last_counts(self):
        """(probe steps, full column compares) of the hash table in the last compression call"""
        probes, compares = C.c_ulonglong(), C.c_ulonglong()
        self.lib.pllhip_compress_last_counts(C.byref(probes), C.byref(compares))
        return probes.value, compares.value

    def compress_last_times(self):
        """(upload, kernels, download) ms of the last compression call"""
        up, kern, down = C.c_double(), C.c_double(), C.c_double()
        self.lib.pllhip_compress_last_times(C.byref(up), C.byref(kern), C.byref(down))
        return up.value, kern.value, down.value

    # --- empirical parameters and alignment statistics ----------------------
    def _take_doubles(self, ptr, n):
        """copy of n doubles the library malloc()ed (freed here), or None when the call returned NULL"""
        if not ptr:
            return None
        out = np.ctypeslib.as_array(ptr, shape=(n,)).copy()
        _libc_free(ptr)
        return out

    def empirical_frequencies(self, partition):
        """pllhip_empirical_frequencies: [states] float64, or None (see errno)"""
        self.errno = 0
        return self._take_doubles(self.lib.pllhip_empirical_frequencies(partition), partition.contents.states)

    def empirical_subst_rates(self, partition):
        """pllhip_empirical_subst_rates: [states * (states - 1) / 2] float64, or None (see errno)"""
        self.errno = 0
        S = partition.contents.states
        return self._take_doubles(self.lib.pllhip_empirical_subst_rates(partition), S * (S - 1) // 2)

    def empirical_invariant_sites(self, partition):
        self.errno = 0
        return self.lib.pllhip_empirical_invariant_sites(partition)

    def msa_compute_stats(self, rows, states, charmap, weights=None, mask=MSA_STATS_ALL, labels=None):
        """pllhip_msa_compute_stats on rows ([T][L] bytes); labels default to t0, t1, ...  Returns a dict of the
        result's fields (lists and float64 arrays; pairs as lists of tuples), or None when the call returned NULL
        (see errno / errmsg)."""
        rows = [bytes(r) for r in rows]
        T, L = len(rows), len(rows[0])
        bufs = [C.create_string_buffer(r, len(r) + 1) for r in rows]
        seqs = (C.c_void_p * T)(*[C.addressof(b) for b in bufs])
        names = [b"t%d" % t for t in range(T)] if labels is None else [bytes(x) for x in labels]
        lab = (C.c_char_p * T)(*names)
        msa = Msa(T, L, seqs, lab)
        cmap = (C.c_ulonglong * 256)(*[int(x) for x in charmap])
        w = None if weights is None else _u32(weights)
        self.errno = 0
        st = self.lib.pllhip_msa_compute_stats(C.byref(msa), states, cmap,
                                               None if w is None else w.ctypes.data_as(c_uint_p), mask)
        if not st:
            return None
        c = st.contents
        npairs = states * (states - 1) // 2
        out = {
            "states": c.states,
            "dup_taxa_pairs": [(c.dup_taxa_pairs[2 * i], c.dup_taxa_pairs[2 * i + 1])
                               for i in range(c.dup_taxa_pairs_count)],
            "dup_seqs_pairs": [(c.dup_seqs_pairs[2 * i], c.dup_seqs_pairs[2 * i + 1])
                               for i in range(c.dup_seqs_pairs_count)],
            "gap_prop": c.gap_prop,
            "gap_seqs": [c.gap_seqs[i] for i in range(c.gap_seqs_count)],
            "gap_cols": [c.gap_cols[i] for i in range(c.gap_cols_count)],
            "inv_prop": c.inv_prop,
            "inv_cols": [c.inv_cols[i] for i in range(c.inv_cols_count)],
            "freqs": np.ctypeslib.as_array(c.freqs, shape=(states,)).copy() if c.freqs else None,
            "subst_rates": np.ctypeslib.as_array(c.subst_rates, shape=(npairs,)).copy() if c.subst_rates else None,
        }
        self.lib.pllhip_msa_destroy_stats(st)
        return out

    def msa_stats_last_times(self):
        """(upload, kernels) ms of the last statistics call"""
        up, kern = C.c_double(), C.c_double()
        self.lib.pllhip_msa_stats_last_times(C.byref(up), C.byref(kern))
        return up.value, kern.value

    def gamma_cats(self, alpha, k, mode=PLL_GAMMA_RATES_MEAN):
        out = np.zeros(k)
        if not self.lib.pll_compute_gamma_cats(alpha, k, out.ctypes.data_as(c_double_p), mode):
            raise RuntimeError(self.errmsg)
        return out


PLLHIP_ERROR_NEWTON_LIMIT, PLLHIP_ERROR_NEWTON_DERIVATIVES = 910, 911
PLLHIP_ERROR_NEWTON_UNSUPPORTED, PLLHIP_ERROR_NEWTON_STUCK = 912, 913
PLLHIP_NEWTON_MAX_ITERATIONS = 1 << 16


class NewtonError(RuntimeError):
    """pllhip_newton_branch / pllhip_newton_branch_multi failed: "[pll_errno] message", and what the call left in its
    outputs -- after PLLHIP_ERROR_NEWTON_LIMIT / _DERIVATIVES the scans made, the length the loop stood at and the
    iterates; untouched (0, nan) where no loop ran"""

    def __init__(self, lib, length, iterations, trail):
        self.errno = lib.errno
        super().__init__(f"[{self.errno}] {lib.errmsg}")
        self.length = length
        self.iterations = iterations
        self.trail = trail[:min(iterations, len(trail))]


class Instance:
    """A partition plus the index bookkeeping of one (tree, model, alignment)."""

    def __init__(self, lib, tips, states, sites, rate_cats, attributes=0, scalers=True,
                 rate_matrices=1, prob_matrices=None, clv_buffers=None):
        self.lib, self.L = lib, lib.lib
        self.tips, self.S, self.N, self.R = tips, states, sites, rate_cats
        inner = tips - 2 if clv_buffers is None else clv_buffers
        nmat = 2 * tips - 3 if prob_matrices is None else prob_matrices
        self.nscalers = inner if scalers else 0
        self.p = self.L.pll_partition_create(tips, inner, states, sites, rate_matrices, nmat,
                                             rate_cats, self.nscalers, attributes)
        if not self.p:
            raise RuntimeError(f"pll_partition_create failed: [{lib.errno}] {lib.errmsg}")
        self.Sp = self.p.contents.states_padded
        self.rate_scalers = bool(attributes & PLL_ATTRIB_RATE_SCALERS)
        # with ascertainment-bias correction every per-site array carries `states` extra patterns
        self.Nalloc = sites + (states if attributes & (PLL_ATTRIB_AB_FLAG | (7 << 5)) else 0)
        self.params = _u32(np.zeros(rate_cats))
        self._keep = []

    def close(self):
        if self.p:
            self.L.pll_partition_destroy(self.p)
            self.p = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def params_p(self):
        return self.params.ctypes.data_as(c_uint_p)

    def set_params_indices(self, indices):
        """per-rate-category parameter-set indices (params_indices / freqs_indices of every kernel
        call; src/tree/treeinfo.c:288-306): category r uses rate matrix indices[r]"""
        idx = _u32(indices)
        assert len(idx) == self.R
        self.params = idx

    # --- model ------------------------------------------------------------
    def set_model(self, subst, freqs, rates, weights=None, idx=0):
        s, f, r = _f64(subst), _f64(freqs), _f64(rates)
        self.L.pll_set_subst_params(self.p, idx, s.ctypes.data_as(c_double_p))
        self.L.pll_set_frequencies(self.p, idx, f.ctypes.data_as(c_double_p))
        self.L.pll_set_category_rates(self.p, r.ctypes.data_as(c_double_p))
        if weights is not None:
            w = _f64(weights)
            self.L.pll_set_category_weights(self.p, w.ctypes.data_as(c_double_p))

    def set_tip_states(self, tip, charmap, seq_bytes):
        m = (C.c_ulonglong * 256)(*[int(x) for x in charmap])
        if not self.L.pll_set_tip_states(self.p, tip, m, bytes(seq_bytes)):
            raise RuntimeError(f"pll_set_tip_states: {self.lib.errmsg}")

    def set_tip_clv(self, tip, clv, padding=0):
        a = _f64(clv)
        if not self.L.pll_set_tip_clv(self.p, tip, a.ctypes.data_as(c_double_p), padding):
            raise RuntimeError(f"pll_set_tip_clv: {self.lib.errmsg}")

    def set_pattern_weights(self, w):
        a = _u32(w)
        self.L.pll_set_pattern_weights(self.p, a.ctypes.data_as(c_uint_p))

    def set_asc(self, asc_type, state_weights=None):
        if not self.L.pll_set_asc_bias_type(self.p, asc_type):
            raise RuntimeError(self.lib.errmsg)
        if state_weights is not None:
            w = _u32(state_weights)
            self.L.pll_set_asc_state_weights(self.p, w.ctypes.data_as(c_uint_p))

    def set_pinv(self, pinv, idx=0):
        if not self.L.pll_update_invariant_sites_proportion(self.p, idx, pinv):
            raise RuntimeError(self.lib.errmsg)

    # --- hot path ---------------------------------------------------------
    def update_pmatrices(self, matrix_indices, brlens, one_by_one=False):
        mi, bl = _u32(matrix_indices), _f64(brlens)
        if one_by_one:      # the reference's treeinfo issues count = 1 per branch
            for k in range(len(mi)):
                if not self.L.pll_update_prob_matrices(
                        self.p, self.params_p,
                        C.cast(mi.ctypes.data + 4 * k, c_uint_p),
                        C.cast(bl.ctypes.data + 8 * k, c_double_p), 1):
                    raise RuntimeError(self.lib.errmsg)
            return
        if not self.L.pll_update_prob_matrices(self.p, self.params_p, mi.ctypes.data_as(c_uint_p),
                                               bl.ctypes.data_as(c_double_p), len(mi)):
            raise RuntimeError(self.lib.errmsg)

    @staticmethod
    def make_ops(op_tuples):
        """op_tuples: (parent_clv, parent_scaler, c1_clv, c1_mat, c1_scaler, c2_clv, c2_mat, c2_scaler)"""
        arr = (Operation * max(1, len(op_tuples)))()
        for k, t in enumerate(op_tuples):
            (arr[k].parent_clv_index, arr[k].parent_scaler_index, arr[k].child1_clv_index,
             arr[k].child1_matrix_index, arr[k].child1_scaler_index, arr[k].child2_clv_index,
             arr[k].child2_matrix_index, arr[k].child2_scaler_index) = [int(x) for x in t]
        return arr

    def update_partials(self, ops, count=None):
        if not isinstance(ops, C.Array):
            count = len(ops)
            ops = self.make_ops(ops)
        self.lib.errno = 0
        self.L.pll_update_partials(self.p, ops, len(ops) if count is None else count)
        if self.lib.errno:
            raise RuntimeError(self.lib.errmsg)

    def edge_lnl(self, pc, psc, cc, csc, matrix, persite=False):
        buf = np.zeros(self.N) if persite else None
        v = self.L.pll_compute_edge_loglikelihood(
            self.p, pc, psc, cc, csc, matrix, self.params_p,
            buf.ctypes.data_as(c_double_p) if persite else None)
        return (v, buf) if persite else v

    def root_lnl(self, clv, sc, persite=False):
        buf = np.zeros(self.N) if persite else None
        v = self.L.pll_compute_root_loglikelihood(
            self.p, clv, sc, self.params_p, buf.ctypes.data_as(c_double_p) if persite else None)
        return (v, buf) if persite else v

    def node_ancestral(self, node, node_sc, other, other_sc, matrix):
        out = np.zeros(self.N * self.S)
        if not self.L.pll_compute_node_ancestral(self.p, node, node_sc, other, other_sc, matrix,
                                                 self.params_p, out.ctypes.data_as(c_double_p)):
            raise RuntimeError(self.lib.errmsg)
        return out.reshape(self.N, self.S)

    def node_ancestral_batch(self, nodes, others, matrices, flags=0, pad=0):
        """pllhip_node_ancestral_batch over the triples (nodes[k], others[k], matrices[k]):
        (states [count][N] uint8, state_probs [count][N], probs [count][N][S] or None).  pad: that many canary
        elements (0xA5 bytes / -7.0) in front of and behind every host array, returned as a fourth value
        `intact` (bool) -- for tests of the bounds of what the library writes"""
        nd, ot, mi = _u32(nodes), _u32(others), _u32(matrices)
        cnt, N, S = len(nd), self.N, self.S
        want = bool(flags & PLLHIP_ANC_PROBS)
        st = np.full((cnt, N + 2 * pad), 0xA5, dtype=np.uint8)
        sp = np.full((cnt, N + 2 * pad), -7.0)
        pr = np.full((cnt, N * S + 2 * pad), -7.0) if want else None

        def ptrs(a, item):
            return (C.c_void_p * max(1, cnt))(*[a.ctypes.data + (k * a.shape[1] + pad) * item for k in range(cnt)])
        self.lib.errno = 0
        if not self.L.pllhip_node_ancestral_batch(self.p, cnt, nd.ctypes.data_as(c_uint_p), ot.ctypes.data_as(c_uint_p),
                                                  mi.ctypes.data_as(c_uint_p), self.params_p, flags, ptrs(st, 1),
                                                  ptrs(sp, 8), ptrs(pr, 8) if want else None):
            raise RuntimeError(f"[{self.lib.errno}] {self.lib.errmsg}")
        out = (st[:, pad:pad + N].copy(), sp[:, pad:pad + N].copy(),
               pr[:, pad:pad + N * S].reshape(cnt, N, S).copy() if want else None)
        if not pad:
            return out
        intact = bool((st[:, :pad] == 0xA5).all() and (st[:, pad + N:] == 0xA5).all() and
                      (sp[:, :pad] == -7.0).all() and (sp[:, pad + N:] == -7.0).all() and
                      (not want or ((pr[:, :pad] == -7.0).all() and (pr[:, pad + N * S:] == -7.0).all())))
        return out + (intact,)

    def alloc_sumtable(self):
        """caller-owned buffer exactly as src/tree/treeinfo.c:336-340 allocates it"""
        n = self.Nalloc * self.R * self.Sp          # src/tree/treeinfo.c:333-337 adds the AB patterns too
        ptr = self.L.pll_aligned_alloc(max(1, n) * 8, self.p.contents.alignment)
        return C.cast(ptr, c_double_p)

    def free_sumtable(self, st):
        self.L.pll_aligned_free(C.cast(st, C.c_void_p))

    def update_sumtable(self, pc, cc, psc, csc, st):
        if not self.L.pll_update_sumtable(self.p, pc, cc, psc, csc, self.params_p, st):
            raise RuntimeError(self.lib.errmsg)

    def derivatives(self, psc, csc, t, st):
        df, ddf = C.c_double(), C.c_double()
        if not self.L.pll_compute_likelihood_derivatives(self.p, psc, csc, t, self.params_p, st,
                                                         C.byref(df), C.byref(ddf)):
            raise RuntimeError(self.lib.errmsg)
        return df.value, ddf.value

    def newton_branch(self, psc, csc, st, start, bl_min, bl_max, tolerance, max_newton):
        """pllhip_newton_branch: (length, iterations, trail) -- the trail holds the first 96 iterates of a longer
        loop -- or raises NewtonError with the library's message"""
        length, its = C.c_double(float("nan")), C.c_uint(0)
        trail = np.zeros(96)
        self.lib.errno = 0
        ok = self.L.pllhip_newton_branch(self.p, psc, csc, self.params_p, st, start, bl_min, bl_max, tolerance,
                                         max_newton, C.byref(length), C.byref(its), trail.ctypes.data_as(c_double_p))
        if not ok:
            raise NewtonError(self.lib, length.value, its.value, trail)
        return length.value, its.value, trail[:its.value]

    def derivatives_multi(self, psc, csc, ts, st):
        """(df[], ddf[]) at several branch lengths from one sumtable scan"""
        t = _f64(ts)
        df, ddf = np.zeros(len(t)), np.zeros(len(t))
        if not self.L.pllhip_compute_likelihood_derivatives_multi(
                self.p, psc, csc, t.ctypes.data_as(c_double_p), len(t), self.params_p, st,
                df.ctypes.data_as(c_double_p), ddf.ctypes.data_as(c_double_p)):
            raise RuntimeError(self.lib.errmsg)
        return df, ddf

    # --- read-back (works for both libraries) -------------------------------
    def get_clv(self, idx):
        n = self.Nalloc * self.R * self.Sp
        out = np.zeros(n)
        if self.lib.is_product:
            if not self.L.pllhip_get_clv(self.p, idx, out.ctypes.data_as(c_double_p)):
                raise RuntimeError(self.lib.errmsg)
        else:
            ptr = self.p.contents.clv[idx]
            out[:] = np.ctypeslib.as_array(ptr, shape=(n,))
        return out.reshape(self.Nalloc, self.R, self.Sp)[:self.N, :, :self.S]

    def get_scaler(self, idx):
        """scaler counts: [site], or [site][rate] with PLL_ATTRIB_RATE_SCALERS"""
        n = self.Nalloc * (self.R if self.rate_scalers else 1)
        out = np.zeros(n, dtype=np.uint32)
        if self.lib.is_product:
            if not self.L.pllhip_get_scaler(self.p, idx, out.ctypes.data_as(c_uint_p)):
                raise RuntimeError(self.lib.errmsg)
        else:
            out[:] = np.ctypeslib.as_array(self.p.contents.scale_buffer[idx], shape=(n,))
        return out[:self.N * (self.R if self.rate_scalers else 1)]

    def get_pmatrix(self, idx):
        if self.lib.is_product:
            self.L.pllhip_sync_to_host(self.p, PLLHIP_SYNC_PMATRIX)
        n = self.R * self.S * self.Sp
        a = np.ctypeslib.as_array(self.p.contents.pmatrix[idx], shape=(n,)).copy()
        return a.reshape(self.R, self.S, self.Sp)[:, :, :self.S]

    def get_sumtable(self, st):
        n = self.Nalloc * self.R * self.Sp
        out = np.zeros(n)
        if self.lib.is_product:
            if not self.L.pllhip_get_sumtable(self.p, st, out.ctypes.data_as(c_double_p)):
                raise RuntimeError(self.lib.errmsg)
        else:
            out[:] = np.ctypeslib.as_array(st, shape=(n,))
        return out.reshape(self.Nalloc, self.R, self.Sp)[:self.N, :, :self.S]

    def counters(self):
        c = Counters()
        self.L.pllhip_get_counters(self.p, C.byref(c))
        return c

    def repeat_stats(self):
        st = RepeatStats()
        self.L.pllhip_repeat_stats(self.p, C.byref(st))
        return st

    # evaluate-only traversals (include/pllhip.h, pllhip_set_transient)
    def set_transient(self, on=True):
        self.L.pllhip_set_transient(self.p, 1 if on else 0)

    def discard_transient(self):
        self.L.pllhip_discard_transient(self.p)

    def transient_stats(self):
        st = TransientStats()
        self.L.pllhip_transient_stats(self.p, C.byref(st))
        return st

    def schedule_stats(self):
        st = ScheduleStats()
        self.L.pllhip_schedule_stats(self.p, C.byref(st))
        return st

    # stores that storing traversals deferred (include/pllhip.h, pllhip_deferred_stats)
    def deferred_stats(self):
        st = DeferredStats()
        self.L.pllhip_deferred_stats(self.p, C.byref(st))
        return st


# ---------------------------------------------------------------------------
# synthetic workloads
# ---------------------------------------------------------------------------
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64(seed, n, start=0):
    """values start .. start+n-1 of the splitmix64 stream started at `seed` (vectorised;
    the stream is counter-based, so any range can be generated on its own)"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * np.arange(start + 1, start + n + 1, dtype=np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def uniform01(seed, n):
    return (splitmix64(seed, n) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def _balanced_pick(t):
    """the tip whose pendant edge tip t splits in a balanced tree: tips 0, 1, 2, 3, ... in turn, starting over
    whenever every existing tip has been split once (3 -> 6 -> 12 -> ... tips: a complete binary tree)"""
    start, size = 3, 3
    while t >= start + size:
        start += size
        size *= 2
    return t - start


class Tree:
    """Unrooted binary tree as index arrays.

    tip i -> CLV i; inner node k -> CLV tips+k, scaler k; every edge has a
    unique P-matrix index 0..2n-4.  `ops` is the post-order
    operation list towards the root edge (root_a, root_b, root_matrix).
    """

    def __init__(self, ntips, seed_topology=42, seed_brlen=43, brlen_range=(0.01, 0.2), ladder=False, balanced=False):
        assert ntips >= 3
        self.ntips = ntips
        self.is_ladder = ladder
        rnd = splitmix64(seed_topology, ntips)
        # edges as [u, v]; start with a star on tips 0,1,2 around inner node n
        edges = [[0, ntips], [1, ntips], [2, ntips]]
        pendant = {0: 0, 1: 1, 2: 2}            # tip -> index of its pendant edge
        for t in range(3, ntips):
            # ladder: always split the pendant edge of the tip added last (a caterpillar);
            # balanced: the pendant edges of the tips in turn (every tip becomes a cherry before any is split twice)
            if ladder:
                e = len(edges) - 1
            elif balanced:
                e = pendant[_balanced_pick(t)]
            else:
                e = int(rnd[t] % np.uint64(len(edges)))
            u, v = edges[e]
            w = ntips + (t - 2)          # new inner node
            edges[e] = [u, w]
            edges.append([w, v])
            edges.append([t, w])
            if u < ntips:                # the split edge was the pendant edge of tip u: it still is (u -- w)
                pendant[u] = e
            elif v < ntips:
                pendant[v] = len(edges) - 2
            pendant[t] = len(edges) - 1
        self.edges = edges
        lo, hi = brlen_range
        self.brlens = lo + (hi - lo) * uniform01(seed_brlen, len(edges))
        self.nedges = len(edges)
        adj = {}
        for k, (u, v) in enumerate(edges):
            adj.setdefault(u, []).append((v, k))
            adj.setdefault(v, []).append((u, k))
        self.adj = adj
        self.set_root_edge(self.nedges - 1 if ntips > 3 else 2)

    def scaler_of(self, node):
        return node - self.ntips if node >= self.ntips else PLL_SCALE_BUFFER_NONE

    def _postorder(self, node, parent, out):
        """iterative post-order of the subtree at `node` seen from `parent`"""
        stack = [(node, parent, False)]
        while stack:
            nd, par, done = stack.pop()
            if nd < self.ntips:
                continue
            kids = [(v, k) for (v, k) in self.adj[nd] if v != par]
            if done:
                (c1, m1), (c2, m2) = kids
                out.append((nd, self.scaler_of(nd), c1, m1, self.scaler_of(c1),
                            c2, m2, self.scaler_of(c2)))
            else:
                stack.append((nd, par, True))
                for v, _ in kids:
                    stack.append((v, nd, False))

    def set_root_edge(self, k):
        u, v = self.edges[k]
        if u < self.ntips:       # keep an inner node on the "parent" side
            u, v = v, u
        self.root_a, self.root_b, self.root_matrix = u, v, k
        ops = []
        self._postorder(v, u, ops)
        self._postorder(u, v, ops)
        self.ops = ops

    def ops_with_scalers(self, use):
        if use:
            return self.ops
        N = PLL_SCALE_BUFFER_NONE
        return [(p, N, a, ma, N, b, mb, N) for (p, _, a, ma, _, b, mb, _) in self.ops]

    def newick(self, labels=None):
        def rec(nd, par, k):
            if nd < self.ntips:
                s = labels[nd] if labels else f"t{nd}"
            else:
                s = "(" + ",".join(rec(v, nd, kk) for (v, kk) in self.adj[nd] if v != par) + ")"
            return s + (f":{self.brlens[k]:.17g}" if k is not None else "")
        root = self.ntips
        return "(" + ",".join(rec(v, root, kk) for (v, kk) in self.adj[root]) + ");"


DNA_GTR_RATES = [1.452176, 0.937951, 0.462880, 0.617729, 1.745312, 1.0]   # blopt-minimal.c:49
DNA_FREQS = [0.17, 0.19, 0.25, 0.39]                                       # spr-round.c:153


def protein_model(seed_rates=46, seed_freqs=47):
    """'LG-shaped' reversible 20-state model: 190 log-normal exchangeabilities
    and Dirichlet(5) frequencies.  The real LG table is not available offline
    (src/util/models_aa.c:29 takes it from libpll), so this is NOT LG."""
    u = uniform01(seed_rates, 380)
    z = np.sqrt(-2.0 * np.log(np.maximum(u[0::2], 1e-300))) * np.cos(2 * np.pi * u[1::2])
    rates = np.exp(z)
    rates[-1] = 1.0
    g = -np.log(np.maximum(uniform01(seed_freqs, 100), 1e-300)).reshape(20, 5).sum(axis=1)
    return rates, g / g.sum()


def codon_model(kappa=2.0, omega=0.2, seed_freqs=48):
    """GY94-shaped 61-state model from the standard genetic code."""
    bases = "TCAG"
    aa = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
    codons = [(a + b + c) for a in bases for b in bases for c in bases]
    sense = [(cd, aa[i]) for i, cd in enumerate(codons) if aa[i] != "*"]
    n = len(sense)
    assert n == 61
    transitions = {("T", "C"), ("C", "T"), ("A", "G"), ("G", "A")}
    rates = []
    for i in range(n):
        for j in range(i + 1, n):
            ci, ai = sense[i]
            cj, aj = sense[j]
            diff = [(x, y) for x, y in zip(ci, cj) if x != y]
            if len(diff) != 1:
                rates.append(0.0)
                continue
            r = 1.0
            if diff[0] in transitions:
                r *= kappa
            if ai != aj:
                r *= omega
            rates.append(r)
    g = -np.log(np.maximum(uniform01(seed_freqs, 61 * 5), 1e-300)).reshape(61, 5).sum(axis=1)
    return np.array(rates), g / g.sum()


def random_codes(ntips, nsites, nstates, seed=44, first_site=0):
    """iid uniform unambiguous state index per (tip, site) -> uint8 [tips][sites];
    sites first_site .. first_site+nsites-1 of the alignment that `seed` defines (a
    rank of a multi-GPU run generates just its slice)"""
    out = np.empty((ntips, nsites), dtype=np.uint8)
    for t in range(ntips):
        out[t] = (splitmix64(seed + 1000003 * t, nsites, first_site) % np.uint64(nstates)).astype(np.uint8)
    return out


def simulated_codes(tree, nsites, nstates, seed=45, scale=1.0):
    """states evolved along `tree` (a Tree) from inner node `ntips` outwards:
    equal-rates process, two site-rate classes; uint8 [tips][sites].  Gives an
    alignment with phylogenetic signal (seed 45)."""
    out = np.empty((tree.ntips, nsites), dtype=np.uint8)
    S = nstates
    rate = np.where(uniform01(seed, nsites) < 0.5, 0.4, 1.6)
    start = (splitmix64(seed + 1, nsites) % np.uint64(S)).astype(np.int64)
    stack = [(tree.ntips, -1, start)]
    while stack:
        node, parent, state = stack.pop()
        if node < tree.ntips:
            out[node] = state.astype(np.uint8)
            continue
        for child, k in tree.adj[node]:
            if child == parent:
                continue
            t = tree.brlens[k] * scale
            pchange = (S - 1.0) / S * (1.0 - np.exp(-S / (S - 1.0) * t * rate))
            u = uniform01(seed + 7919 * (k + 1), nsites)
            jump = 1 + (splitmix64(seed + 104729 * (k + 1), nsites) % np.uint64(S - 1)).astype(np.int64)
            stack.append((child, node, np.where(u < pchange, (state + jump) % S, state)))
    return out


def utree_splits(tree):
    """the splits of a pll_utree_t (a POINTER(UTree)) as a set of frozensets of tip clv indices: per edge the
    side without the smallest tip index (so two trees over the same tips compare as sets)"""
    t = tree.contents
    tips = [t.nodes[i].contents.clv_index for i in range(t.tip_count)]
    low = min(tips)
    below = {}

    def side(rec):
        """tips behind the record `rec` (the subtree its `back` leads away from)"""
        key = C.addressof(rec.contents)
        if key in below:
            return below[key]
        out, stack = set(), [rec]
        while stack:
            r = stack.pop()
            b = r.contents.back
            if not b.contents.next:
                out.add(b.contents.clv_index)
                continue
            n = b.contents.next
            while C.addressof(n.contents) != C.addressof(b.contents):
                stack.append(n)
                n = n.contents.next
        below[key] = frozenset(out)
        return below[key]

    splits = set()
    for i in range(t.tip_count + t.inner_count):
        r = t.nodes[i]
        recs = [r]
        if r.contents.next:
            n = r.contents.next
            while C.addressof(n.contents) != C.addressof(r.contents):
                recs.append(n)
                n = n.contents.next
        for rec in recs:
            s = side(rec)
            splits.add(s if low not in s else frozenset(tips) - s)
    return splits


SUPPORT_FBP, SUPPORT_TBE = 0, 1
_libc_free = C.CDLL(None).free
_libc_free.restype, _libc_free.argtypes = None, [C.c_void_p]


def consensus_needs(lib, tree_count, threshold):
    """(need_major, need_minor) of pllhip_consensus_needs, or None"""
    a, b = C.c_uint(0), C.c_uint(0)
    return (a.value, b.value) if lib.lib.pllhip_consensus_needs(tree_count, threshold, C.byref(a), C.byref(b)) else None

PLL_ERROR_MEM_ALLOC, PLL_ERROR_PARAM_INVALID, PLL_ERROR_TREE_INVALID = 112, 113, 133
PLL_ERROR_HIP_RUNTIME, PLL_ERROR_HIP_NODEVICE = 900, 901


class TreeSet:
    """pllhip_treeset_* (include/pllhip.h): a set of binary trees over the same tips.  Trees go in as Newick strings
    (parsed by the library) or as POINTER(UTree); a failed call returns None / False with lib.errno set."""

    def __init__(self, lib, tip_count, labels=None):
        self.lib, self.L, self.T = lib, lib.lib, tip_count
        arr = None
        if labels is not None:
            arr = (C.c_char_p * len(labels))(*[None if l is None else l.encode() for l in labels])
        self.h = self.L.pllhip_treeset_create(tip_count, arr)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self.h:
            self.L.pllhip_treeset_destroy(self.h)
            self.h = None

    @property
    def count(self):
        return self.L.pllhip_treeset_count(self.h)

    @property
    def words(self):
        return (self.T + 31) // 32

    def _with_tree(self, tree, call):
        """call(POINTER(UTree)) on a Newick string or a tree"""
        if not isinstance(tree, str):
            return call(tree)
        t = self.L.pll_utree_parse_newick_string(tree.encode())
        if not t:
            raise ValueError(f"cannot parse {tree[:60]!r}: {self.lib.errmsg}")
        try:
            return call(t)
        finally:
            self.L.pll_utree_destroy(t, None)

    def add(self, tree):
        return bool(self._with_tree(tree, lambda t: self.L.pllhip_treeset_add(self.h, t)))

    def plan(self, index):
        """(order, lo, hi, program [2T-3, 2], deepest stack) of tree `index`, or None"""
        T = self.T
        order, lo, hi = np.zeros(T - 1, np.uint32), np.zeros(T - 3, np.uint32), np.zeros(T - 3, np.uint32)
        prog, deepest = np.zeros((2 * T - 3, 2), np.uint32), C.c_uint(0)
        ok = self.L.pllhip_treeset_plan(self.h, index, order.ctypes.data_as(c_uint_p), lo.ctypes.data_as(c_uint_p),
                                        hi.ctypes.data_as(c_uint_p), prog.ctypes.data_as(c_uint_p), C.byref(deepest))
        return (order, lo, hi, prog, deepest.value) if ok else None

    def splits(self, index):
        out = np.zeros((self.T - 3, self.words), np.uint32)
        return out if self.L.pllhip_treeset_splits(self.h, index, out.ctypes.data_as(c_uint_p)) else None

    def rf_matrix(self):
        B = self.count
        out = np.zeros((B, B), np.uint32)
        return out if self.L.pllhip_treeset_rf_matrix(self.h, out.ctypes.data_as(c_uint_p)) else None

    def rf_to(self, ref):
        out = np.zeros(self.count, np.uint32)
        ok = self._with_tree(ref, lambda t: self.L.pllhip_treeset_rf_to(self.h, t, out.ctypes.data_as(c_uint_p)))
        return out if ok else None

    def support(self, ref, kind, with_map=False):
        """(support [T-3], the integers behind it [T-3]) or None; with_map: also, per split, the clv indices of the
        tips behind the mapped record's back pointer (the side of the edge away from the record)"""
        R = self.T - 3
        out, nodes = np.zeros(R, np.float64), (C.POINTER(UNode) * R)()
        sides = []

        def call(t):
            ok = self.L.pllhip_treeset_support(self.h, t, kind, out.ctypes.data_as(c_double_p), nodes if with_map else None)
            if ok and with_map:
                for rec in nodes:
                    tips, stack = set(), [rec.contents.back]
                    while stack:
                        r = stack.pop()
                        if not r.contents.next:
                            tips.add(r.contents.label.decode() if r.contents.label else r.contents.node_index)
                        else:
                            stack += [r.contents.next.contents.back, r.contents.next.contents.next.contents.back]
                    sides.append(frozenset(tips))
            return ok

        if not self._with_tree(ref, call):
            return None
        sums = np.zeros(R, np.uint64)
        self.L.pllhip_treeset_last_sums(sums.ctypes.data_as(C.POINTER(C.c_ulonglong)), R)
        return (out, sums, sides) if with_map else (out, sums)

    def consensus(self, threshold):
        """(words [K, len], trees [K], support [K]) of the consensus split system in rank order, or None"""
        R, K = self.T - 3, C.c_uint(0)
        words, trees, support = np.zeros((R, self.words), np.uint32), np.zeros(R, np.uint32), np.zeros(R, np.float64)
        ok = self.L.pllhip_treeset_consensus(self.h, threshold, C.byref(K), words.ctypes.data_as(c_uint_p),
                                             trees.ctypes.data_as(c_uint_p), support.ctypes.data_as(c_double_p))
        return (words[:K.value].copy(), trees[:K.value].copy(), support[:K.value].copy()) if ok else None

    def _newick_of(self, tree):
        if not tree:
            return None
        text = self.L.pll_utree_export_newick(tree.contents.vroot, None)
        out = C.string_at(text).decode()
        _libc_free(text)
        self.L.pll_utree_destroy(tree, None)
        return out

    def consensus_newick(self, threshold):
        """the consensus tree as Newick, supports as inner labels; None on failure"""
        return self._newick_of(self.L.pllhip_treeset_consensus_tree(self.h, threshold))

    def newick_from_splits(self, words, support=None):
        """the tree of a system of compatible splits (host only), as Newick; None on failure"""
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, self.words)
        sup = None if support is None else np.ascontiguousarray(support, dtype=np.float64)
        return self._newick_of(self.L.pllhip_treeset_tree_from_splits(
            self.h, len(words), words.ctypes.data_as(c_uint_p), None if sup is None else sup.ctypes.data_as(c_double_p)))

    def last_consensus_counts(self):
        a, b = C.c_ulonglong(0), C.c_ulonglong(0)
        self.L.pllhip_treeset_last_consensus_counts(C.byref(a), C.byref(b))
        return a.value, b.value

    def last_times(self):
        up, kern, down = C.c_double(0), C.c_double(0), C.c_double(0)
        self.L.pllhip_treeset_last_times(C.byref(up), C.byref(kern), C.byref(down))
        return up.value, kern.value, down.value

    def last_counts(self):
        probes, compares = C.c_ulonglong(0), C.c_ulonglong(0)
        self.L.pllhip_treeset_last_counts(C.byref(probes), C.byref(compares))
        return probes.value, compares.value


class SiteLikelihoods:
    """pllhip_sitelh_* (include/pllhip.h): per-pattern log-likelihoods of several trees on the device.  A failed call
    returns None / False with lib.errno set."""

    def __init__(self, lib, patterns, weights=None):
        self.lib, self.L, self.S = lib, lib.lib, patterns
        w = None if weights is None else _u32(weights)
        self.h = self.L.pllhip_sitelh_create(patterns, None if w is None else w.ctypes.data_as(c_uint_p))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self.h:
            self.L.pllhip_sitelh_destroy(self.h)
            self.h = None

    @property
    def count(self):
        return self.L.pllhip_sitelh_count(self.h)

    def add(self, row):
        """appends a host row; the tree index, or None"""
        r = _f64(row)
        assert r.shape == (self.S,)
        k = self.L.pllhip_sitelh_add(self.h, r.ctypes.data_as(c_double_p))
        return None if k < 0 else k

    def add_edge(self, tree, offset, inst, pc, psc, cc, csc, matrix):
        """the edge log-likelihood of Instance `inst` with its per-pattern values left in row `tree` at `offset`;
        the log-likelihood, or None"""
        v = C.c_double(0.0)
        ok = self.L.pllhip_sitelh_add_edge(self.h, tree, offset, inst.p, pc, psc, cc, csc, matrix, inst.params_p,
                                           C.byref(v))
        return v.value if ok else None

    def get(self, tree):
        out = np.zeros(self.S)
        return out if self.L.pllhip_sitelh_get(self.h, tree, out.ctypes.data_as(c_double_p)) else None

    def rell(self, replicates, seed, flags=0, batch=0):
        """pllhip_sitelh_rell as a Rell, or None"""
        params = RellParams(replicates, seed, flags, batch)
        rp = self.L.pllhip_sitelh_rell(self.h, C.byref(params))
        if not rp:
            return None
        try:
            r, out = rp.contents, Rell()
            T, B = r.trees, r.replicates
            out.trees, out.replicates, out.best, out.batch = T, B, r.best, r.batch
            out.lnl = np.ctypeslib.as_array(r.lnl, (T,)).copy()
            out.bp_count = np.ctypeslib.as_array(r.bp_count, (T,)).copy()
            out.kh_count = np.ctypeslib.as_array(r.kh_count, (T,)).copy()
            out.sh_count = np.ctypeslib.as_array(r.sh_count, (T,)).copy()
            out.elw = np.ctypeslib.as_array(r.elw, (T,)).copy()
            out.R = np.ctypeslib.as_array(r.replicate_lnl, (B, T)).copy() if r.replicate_lnl else None
        finally:
            self.L.pllhip_rell_destroy(rp)
        a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
        self.L.pllhip_rell_last_times(C.byref(a), C.byref(b), C.byref(c))
        out.times = (a.value, b.value, c.value)
        return out

    def au(self, replicates, seed, scale=None, flags=0, batch=0, scales=None):
        """pllhip_sitelh_au as an Au, or None; scale = the r_k (None: the library's ten), scales = K where it is to
        differ from len(scale)"""
        r = None if scale is None else _f64(scale)
        K = (0 if r is None else len(r)) if scales is None else scales
        params = AuParams(replicates, K, None if r is None else r.ctypes.data_as(c_double_p), seed, flags, batch)
        rp = self.L.pllhip_sitelh_au(self.h, C.byref(params))
        if not rp:
            return None
        try:
            a, out = rp.contents, Au()
            T, B, K = a.trees, a.replicates, a.scales
            out.trees, out.replicates, out.scales, out.best, out.batch = T, B, K, a.best, a.batch
            out.lnl = np.ctypeslib.as_array(a.lnl, (T,)).copy()
            out.draws = np.ctypeslib.as_array(a.draws, (K,)).copy()
            out.bp_count = np.ctypeslib.as_array(a.bp_count, (K, T)).copy()
            for name in ("p_au", "d", "c", "se", "rss", "used"):
                setattr(out, name, np.ctypeslib.as_array(getattr(a, name), (T,)).copy())
            out.R = np.ctypeslib.as_array(a.replicate_lnl, (K, B, T)).copy() if a.replicate_lnl else None
        finally:
            self.L.pllhip_au_destroy(rp)
        x, y, z = C.c_double(0), C.c_double(0), C.c_double(0)
        self.L.pllhip_au_last_times(C.byref(x), C.byref(y), C.byref(z))
        out.times = (x.value, y.value, z.value)
        return out


class SiteCat:
    """a pllhip_sitecat_t: SiteCat.edge(inst, parent, parent_scaler, child, child_scaler, matrix) or
    SiteCat.from_table(lib, g, pattern_weights=None, weights=None); raises RuntimeError with the library's message"""

    def __init__(self, lib, handle):
        if not handle:
            raise RuntimeError(f"[{lib.errno}] {lib.errmsg}")
        self.lib, self.L, self.h = lib, lib.lib, handle
        self.sites, self.cats = self.L.pllhip_sitecat_sites(handle), self.L.pllhip_sitecat_categories(handle)

    @classmethod
    def edge(cls, inst, pc_, psc, cc, csc, matrix, params=None):
        inst.lib.errno = 0
        prm = inst.params_p if params is None else _u32(params).ctypes.data_as(c_uint_p)
        return cls(inst.lib, inst.L.pllhip_sitecat_edge(inst.p, pc_, psc, cc, csc, matrix, prm))

    @classmethod
    def from_table(cls, lib, g, pattern_weights=None, weights=None):
        g = _f64(g)
        m = _u32(pattern_weights) if pattern_weights is not None else None
        w = _f64(weights) if weights is not None else None
        lib.errno = 0
        return cls(lib, lib.lib.pllhip_sitecat_from_table(g.shape[0], g.shape[1], g.ctypes.data_as(c_double_p),
                                                          m.ctypes.data_as(c_uint_p) if m is not None else None,
                                                          w.ctypes.data_as(c_double_p) if w is not None else None))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self.h:
            self.L.pllhip_sitecat_destroy(self.h)
            self.h = None

    def table(self):
        """(rate_part [sites][cats], inv_part [sites][cats], counts [sites])"""
        a, b = np.zeros((self.sites, self.cats)), np.zeros((self.sites, self.cats))
        c = np.zeros(self.sites, dtype=np.uint32)
        if not self.L.pllhip_sitecat_table(self.h, a.ctypes.data_as(c_double_p), b.ctypes.data_as(c_double_p),
                                           c.ctypes.data_as(c_uint_p)):
            raise RuntimeError(self.lib.errmsg)
        return a, b, c

    def posteriors(self, weights=None, flags=0):
        w = _f64(weights) if weights is not None else None
        self.lib.errno = 0
        ptr = self.L.pllhip_sitecat_posteriors(self.h, w.ctypes.data_as(c_double_p) if w is not None else None, flags)
        if not ptr:
            raise RuntimeError(f"[{self.lib.errno}] {self.lib.errmsg}")
        try:
            return SitePosteriors(ptr.contents)
        finally:
            self.L.pllhip_site_posteriors_destroy(ptr)

    def em_weights(self, epsilon, max_iterations, start=None):
        s = _f64(start) if start is not None else None
        prm = SiteCatEmParams(s.ctypes.data_as(c_double_p) if s is not None else None, epsilon, max_iterations)
        w, tw, tl = np.zeros(self.cats), np.zeros((SITECAT_TRAIL_MAX, self.cats)), np.zeros(SITECAT_TRAIL_MAX)
        ll, its = C.c_double(0.0), C.c_uint(0)
        self.lib.errno = 0
        if not self.L.pllhip_sitecat_em_weights(self.h, C.byref(prm), w.ctypes.data_as(c_double_p), C.byref(ll),
                                                C.byref(its), tw.ctypes.data_as(c_double_p),
                                                tl.ctypes.data_as(c_double_p)):
            raise RuntimeError(f"[{self.lib.errno}] {self.lib.errmsg}")
        fit, n = EmFit(), min(its.value + 1, SITECAT_TRAIL_MAX)
        fit.weights, fit.loglh, fit.iterations = w, ll.value, its.value
        fit.trail_weights, fit.trail_loglh = tw[:n].copy(), tl[:n].copy()
        return fit

    def last_times(self):
        """(table_ms, posterior_ms, em_ms) of this thread's last calls"""
        t = [C.c_double(0.0) for _ in range(3)]
        self.L.pllhip_sitecat_last_times(*[C.byref(x) for x in t])
        return tuple(x.value for x in t)


class EdgePairs:
    """a pllhip_edge_pairs_t: `with EdgePairs.edge(inst, parent, parent_scaler, child, child_scaler, matrix, flags) as ep`
    gives numpy copies F, pairs [cats][S][S], posterior [cats], differ [sites] or None, weight_sum, dropped; raises
    RuntimeError with the library's message"""

    def __init__(self, lib, ptr):
        if not ptr:
            raise RuntimeError(f"[{lib.errno}] {lib.errmsg}")
        self.lib, self.L, self.ptr = lib, lib.lib, ptr
        r = ptr.contents
        S, R, N = r.states, r.cats, r.sites
        self.states, self.cats, self.sites = S, R, N
        self.F = np.ctypeslib.as_array(r.F, shape=(R, S, S)).copy()
        self.pairs = np.ctypeslib.as_array(r.pairs, shape=(R, S, S)).copy()
        self.posterior = np.ctypeslib.as_array(r.posterior, shape=(R,)).copy()
        self.differ = (np.ctypeslib.as_array(r.differ, shape=(N,)).copy() if N else np.zeros(0)) if r.differ else None
        self.weight_sum, self.dropped = r.weight_sum, r.dropped

    @classmethod
    def edge(cls, inst, pc_, psc, cc, csc, matrix, flags=0, params=None):
        inst.lib.errno = 0
        prm = inst.params_p if params is None else _u32(params).ctypes.data_as(c_uint_p)
        return cls(inst.lib, inst.L.pllhip_substmap_edge(inst.p, pc_, psc, cc, csc, matrix, prm, flags))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self.ptr:
            self.L.pllhip_edge_pairs_destroy(self.ptr)
            self.ptr = None

    def last_times(self):
        """(scale_ms, pairs_ms, reduce_ms) of this thread's last call"""
        t = [C.c_double(0.0) for _ in range(3)]
        self.L.pllhip_substmap_last_times(*[C.byref(x) for x in t])
        return tuple(x.value for x in t)


def substmap_counts(lib, eigenvecs, inv_eigenvecs, eigenvals, tau, F):
    """pllhip_substmap_counts -> (counts [S][S], dwell [S]); eigenvecs / inv_eigenvecs [S][Sp] in libpll's storage"""
    ev, iv, ew, F = _f64(eigenvecs), _f64(inv_eigenvecs), _f64(eigenvals), _f64(F)
    S, Sp = F.shape[0], ev.shape[1]
    counts, dwell = np.zeros((S, S)), np.zeros(S)
    lib.errno = 0
    if not lib.lib.pllhip_substmap_counts(S, Sp, ev.ctypes.data_as(c_double_p), iv.ctypes.data_as(c_double_p),
                                          ew.ctypes.data_as(c_double_p), tau, F.ctypes.data_as(c_double_p),
                                          counts.ctypes.data_as(c_double_p), dwell.ctypes.data_as(c_double_p)):
        raise RuntimeError(f"[{lib.errno}] {lib.errmsg}")
    return counts, dwell


class DistMat:
    """pllhip_distmat_t (include/pllhip.h): made by distances_partition / distances_msa / distmat_from_host below.
    A failed call returns None / False with lib.errno set."""

    def __init__(self, lib, handle, states=0):
        self.lib, self.L, self.h, self.S = lib, lib.lib, handle, states
        self.T = self.L.pllhip_distmat_size(handle)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self.h:
            self.L.pllhip_distmat_destroy(self.h)
            self.h = None

    def matrix(self):
        out = np.zeros((self.T, self.T))
        return out if self.L.pllhip_distmat_get(self.h, out.ctypes.data_as(c_double_p)) else None

    def compared(self):
        out = np.zeros((self.T, self.T), np.uint32)
        return out if self.L.pllhip_distmat_compared(self.h, out.ctypes.data_as(c_uint_p)) else None

    def counts(self, i, j):
        """N_ij [S][S] int32, or None (needs DIST_KEEP_COUNTS)"""
        out = np.zeros((self.S, self.S), np.int32)
        return out if self.L.pllhip_distmat_counts(self.h, i, j, out.ctypes.data_as(C.POINTER(C.c_int))) else None

    @property
    def no_overlap(self):
        return self.L.pllhip_distmat_no_overlap(self.h)

    def nj_joins(self):
        """(slots, lengths): T - 3 rounds of (i, j) / (l_i, l_j), then the last three slots and lengths; or None"""
        n = 2 * (self.T - 3) + 3
        slots, lengths = np.zeros(n, np.uint32), np.zeros(n)
        ok = self.L.pllhip_distmat_nj_joins(self.h, slots.ctypes.data_as(c_uint_p), lengths.ctypes.data_as(c_double_p))
        return (slots, lengths) if ok else None

    def nj(self, labels=None):
        """the neighbour-joining tree as POINTER(UTree) (the caller destroys it), or None"""
        arr = None
        if labels is not None:
            arr = (C.c_char_p * len(labels))(*[l if isinstance(l, bytes) else l.encode() for l in labels])
        t = self.L.pllhip_distmat_nj(self.h, arr)
        return t if t else None

    def last_times(self):
        """(upload, codes, counts, estimate, nj) ms of this thread's last calls"""
        v = [C.c_double(0) for _ in range(5)]
        self.L.pllhip_distances_last_times(*[C.byref(x) for x in v])
        return tuple(x.value for x in v)


def _dist_params(method, flags, min_dist, max_dist, budget_bytes, chunk_columns):
    return DistParams(method, flags, min_dist, max_dist, budget_bytes, chunk_columns)


def distances_partition(lib, partition, method=DIST_P, flags=0, min_dist=0.0, max_dist=0.0, budget_bytes=0,
                        chunk_columns=0):
    """pllhip_distances_partition as a DistMat, or None"""
    params = _dist_params(method, flags, min_dist, max_dist, budget_bytes, chunk_columns)
    lib.errno = 0
    h = lib.lib.pllhip_distances_partition(partition, C.byref(params))
    return DistMat(lib, h, partition.contents.states) if h else None


def distances_msa(lib, rows, states, charmap, weights=None, method=DIST_P, flags=0, min_dist=0.0, max_dist=0.0,
                  budget_bytes=0, chunk_columns=0):
    """pllhip_distances_msa on rows ([T][L] bytes) as a DistMat, or None"""
    rows = [bytes(r) for r in rows]
    T, L = len(rows), len(rows[0])
    bufs = [C.create_string_buffer(r, len(r) + 1) for r in rows]
    seqs = (C.c_void_p * T)(*[C.addressof(b) for b in bufs])
    msa = Msa(T, L, seqs, None)
    cmap = (C.c_ulonglong * 256)(*[int(x) for x in charmap])
    w = None if weights is None else _u32(weights)
    params = _dist_params(method, flags, min_dist, max_dist, budget_bytes, chunk_columns)
    lib.errno = 0
    h = lib.lib.pllhip_distances_msa(C.byref(msa), states, cmap, None if w is None else w.ctypes.data_as(c_uint_p),
                                     C.byref(params))
    return DistMat(lib, h, states) if h else None


def distmat_from_host(lib, matrix):
    """pllhip_distmat_from_host as a DistMat, or None"""
    m = _f64(matrix)
    lib.errno = 0
    h = lib.lib.pllhip_distmat_from_host(m.shape[0], m.ctypes.data_as(c_double_p))
    return DistMat(lib, h) if h else None


def bootstrap_weights(lib, weights, patterns, seed, first, count):
    """pllhip_bootstrap_weights: [count][patterns] uint32, or None"""
    w = None if weights is None else _u32(weights)
    out = np.zeros((count, patterns), np.uint32)
    ok = lib.lib.pllhip_bootstrap_weights(None if w is None else w.ctypes.data_as(c_uint_p), patterns, seed, first,
                                          count, out.ctypes.data_as(c_uint_p))
    return out if ok else None


def multiscale_weights(lib, weights, patterns, seed, scale_index, draws, first, count):
    """pllhip_multiscale_weights: [count][patterns] uint32, or None"""
    w = None if weights is None else _u32(weights)
    out = np.zeros((count, patterns), np.uint32)
    ok = lib.lib.pllhip_multiscale_weights(None if w is None else w.ctypes.data_as(c_uint_p), patterns, seed,
                                           scale_index, draws, first, count, out.ctypes.data_as(c_uint_p))
    return out if ok else None


def tree_edges(tree, root=None):
    """the edges of a Tree directed away from inner node `root` (default: the first inner node):
    (parent, child, matrix) index arrays, depth-first"""
    root = tree.ntips if root is None else root
    parent, child, matrix = [], [], []
    stack = [(root, -1)]
    while stack:
        node, came = stack.pop()
        if node < tree.ntips:
            continue
        for v, k in tree.adj[node]:
            if v != came:
                parent.append(node)
                child.append(v)
                matrix.append(k)
                stack.append((v, node))
    return _u32(parent), _u32(child), _u32(matrix)


def _sim_params(seed, sites, replicates, first_site, first_replicate, flags, alphabet):
    a = None if alphabet is None else (alphabet if isinstance(alphabet, bytes) else alphabet.encode())
    return SimParams(seed, first_site, sites, first_replicate, replicates, flags, a)


def _sim_out(inst, rows, sites, replicates, canary):
    shape = (replicates, rows, sites)
    return np.zeros(shape, dtype=np.uint8) if canary is None else np.full(shape, canary, dtype=np.uint8)


def simulate_edges(inst, root, parent, child, matrix, seed, sites, replicates=1, first_site=0, first_replicate=0,
                   flags=0, alphabet=None, node_count=None, params_indices=None, out=None):
    """pllhip_simulate_edges on an Instance with the matrices as they stand: uint8 [replicates][rows][sites], rows =
    tips, or node_count with PLLHIP_SIM_INNER; raises RuntimeError with the library's message.  `out`: the array to
    fill (left as it is on failure)."""
    pa, ch, mi = _u32(parent), _u32(child), _u32(matrix)
    nodes = inst.tips + inst.p.contents.clv_buffers if node_count is None else node_count
    rows = nodes if flags & PLLHIP_SIM_INNER else inst.tips
    if out is None:
        out = _sim_out(inst, rows, sites, replicates, None)
    prm = _sim_params(seed, sites, replicates, first_site, first_replicate, flags, alphabet)
    idx = inst.params if params_indices is None else _u32(params_indices)
    if not inst.L.pllhip_simulate_edges(inst.p, C.byref(prm), root, len(pa), pa.ctypes.data_as(c_uint_p),
                                        ch.ctypes.data_as(c_uint_p), mi.ctypes.data_as(c_uint_p),
                                        idx.ctypes.data_as(c_uint_p), nodes, out.ctypes.data_as(C.POINTER(C.c_ubyte))):
        raise RuntimeError(inst.lib.errmsg)
    return out


def simulate_utree(inst, root, seed, sites, replicates=1, first_site=0, first_replicate=0, flags=0, alphabet=None,
                   update_matrices=True, out=None):
    """pllhip_simulate_utree from `root` (a POINTER(UNode) at an inner node)"""
    rows = inst.tips + inst.p.contents.clv_buffers if flags & PLLHIP_SIM_INNER else inst.tips
    if out is None:
        out = _sim_out(inst, rows, sites, replicates, None)
    prm = _sim_params(seed, sites, replicates, first_site, first_replicate, flags, alphabet)
    if not inst.L.pllhip_simulate_utree(inst.p, C.byref(prm), root, inst.params_p, 1 if update_matrices else 0,
                                        out.ctypes.data_as(C.POINTER(C.c_ubyte))):
        raise RuntimeError(inst.lib.errmsg)
    return out


def simulate_last_times(lib):
    """(tables_ms, kernel_ms, copy_ms, chunks) of this thread's last simulation"""
    a, b, c, n = C.c_double(0), C.c_double(0), C.c_double(0), C.c_ulonglong(0)
    lib.lib.pllhip_simulate_last_times(C.byref(a), C.byref(b), C.byref(c), C.byref(n))
    return a.value, b.value, c.value, n.value


def _ancs_params(seed, replicates, first_replicate, flags, alphabet):
    a = None if alphabet is None else (alphabet if isinstance(alphabet, bytes) else alphabet.encode())
    return AncSampleParams(seed, first_replicate, replicates, flags, a)


def sample_ancestral_edges(inst, root_edge, parent, child, matrix, seed, replicates=1, first_replicate=0, flags=0,
                           alphabet=None, node_count=None, freqs_indices=None, out=None, component=None):
    """pllhip_sample_ancestral_edges on an Instance whose vectors point towards root_edge = (root node, root scaler,
    other node, other scaler): (out uint8 [replicates][node_count][sites], component [replicates][sites], dropped);
    raises RuntimeError with the library's message.  `out`, `component`: the arrays to fill (left as they are on
    failure)."""
    pa, ch, mi = _u32(parent), _u32(child), _u32(matrix)
    nodes = inst.tips + inst.p.contents.clv_buffers if node_count is None else node_count
    if out is None:
        out = np.zeros((replicates, nodes, inst.N), dtype=np.uint8)
    if component is None:
        component = np.zeros((replicates, inst.N), dtype=np.uint8)
    prm = _ancs_params(seed, replicates, first_replicate, flags, alphabet)
    idx = inst.params if freqs_indices is None else _u32(freqs_indices)
    dropped = C.c_ulonglong(0)
    ubyte_p = C.POINTER(C.c_ubyte)
    rn, rs, on, os_ = root_edge
    if not inst.L.pllhip_sample_ancestral_edges(inst.p, C.byref(prm), rn, rs, on, os_, len(pa), pa.ctypes.data_as(c_uint_p),
                                                ch.ctypes.data_as(c_uint_p), mi.ctypes.data_as(c_uint_p),
                                                idx.ctypes.data_as(c_uint_p), nodes, out.ctypes.data_as(ubyte_p),
                                                component.ctypes.data_as(ubyte_p), C.byref(dropped)):
        raise RuntimeError(inst.lib.errmsg)
    return out, component, dropped.value


def sample_ancestral_utree(inst, root, seed, replicates=1, first_replicate=0, flags=0, alphabet=None):
    """pllhip_sample_ancestral_utree from `root` (a POINTER(UNode) at an inner node)"""
    nodes = inst.tips + inst.p.contents.clv_buffers
    out = np.zeros((replicates, nodes, inst.N), dtype=np.uint8)
    component = np.zeros((replicates, inst.N), dtype=np.uint8)
    prm = _ancs_params(seed, replicates, first_replicate, flags, alphabet)
    dropped = C.c_ulonglong(0)
    ubyte_p = C.POINTER(C.c_ubyte)
    if not inst.L.pllhip_sample_ancestral_utree(inst.p, C.byref(prm), root, inst.params_p, out.ctypes.data_as(ubyte_p),
                                                component.ctypes.data_as(ubyte_p), C.byref(dropped)):
        raise RuntimeError(inst.lib.errmsg)
    return out, component, dropped.value


def ancsample_last_times(lib):
    """(table_ms, kernel_ms, copy_ms, chunks) of this thread's last pllhip_sample_ancestral_edges"""
    a, b, c, n = C.c_double(0), C.c_double(0), C.c_double(0), C.c_ulonglong(0)
    lib.lib.pllhip_ancsample_last_times(C.byref(a), C.byref(b), C.byref(c), C.byref(n))
    return a.value, b.value, c.value, n.value


def history_rate_table(lib, eigenvecs, inv_eigenvecs, eigenvals, K, states=None):
    """pllhip_history_rate_table -> (mu, Rpow [K][S][S]); eigenvecs / inv_eigenvecs [S][Sp] in libpll's storage"""
    ev, iv, ew = _f64(eigenvecs), _f64(inv_eigenvecs), _f64(eigenvals)
    S, Sp = (ev.shape[0] if states is None else states), ev.shape[1]
    mu, rpow = C.c_double(0.0), np.zeros((max(K, 1), S, S))
    lib.errno = 0
    if not lib.lib.pllhip_history_rate_table(S, Sp, ev.ctypes.data_as(c_double_p), iv.ctypes.data_as(c_double_p),
                                             ew.ctypes.data_as(c_double_p), K, C.byref(mu), rpow.ctypes.data_as(c_double_p)):
        raise RuntimeError(f"[{lib.errno}] {lib.errmsg}")
    return mu.value, rpow


def history_poisson(lib, lam):
    """pllhip_history_poisson -> pois [K]"""
    pois, K = np.zeros(PLLHIP_HIST_MAX_TABLE), C.c_uint(0)
    lib.errno = 0
    if not lib.lib.pllhip_history_poisson(lam, pois.ctypes.data_as(c_double_p), C.byref(K)):
        raise RuntimeError(f"[{lib.errno}] {lib.errmsg}")
    return pois[:K.value].copy()


def history_summary(lib, tau, counts_int, units):
    """pllhip_history_summary of one (replicate, branch): counts_int uint64 [S][S], units uint64 [R][S], tau [R] ->
    (counts [S][S], dwell [S], total)"""
    ull_p = C.POINTER(C.c_ulonglong)
    tau = _f64(tau)
    ci, un = np.ascontiguousarray(counts_int, dtype=np.uint64), np.ascontiguousarray(units, dtype=np.uint64)
    S, R = ci.shape[0], un.shape[0]
    counts, dwell, total = np.zeros((S, S)), np.zeros(S), C.c_double(0.0)
    lib.errno = 0
    if not lib.lib.pllhip_history_summary(S, R, tau.ctypes.data_as(c_double_p), ci.ctypes.data_as(ull_p),
                                          un.ctypes.data_as(ull_p), counts.ctypes.data_as(c_double_p),
                                          dwell.ctypes.data_as(c_double_p), C.byref(total)):
        raise RuntimeError(f"[{lib.errno}] {lib.errmsg}")
    return counts, dwell, total.value


class Histories:
    """what pllhip_sample_histories_* returns, edges in the order of the list: out uint8 [replicates][node_count][sites],
    component [replicates][sites], dropped, counts uint64 [replicates][edges][S][S], units uint64
    [replicates][edges][R][S], changes uint8 [replicates][edges][sites] or None, dropped_edges uint64
    [replicates][edges], and for the utree form edge_matrix [edges]"""


def sample_histories_edges(inst, root_edge, parent, child, matrix, lengths, seed, replicates=1, first_replicate=0, flags=0,
                           alphabet=None, node_count=None, freqs_indices=None, params_indices=None, want_out=True,
                           want_component=True, fill=0):
    """pllhip_sample_histories_edges on an Instance whose vectors point towards root_edge = (root node, root scaler,
    other node, other scaler) -> Histories; raises RuntimeError with the library's message, with h.partial holding the
    arrays as the call left them (initialised to `fill`)."""
    pa, ch, mi = _u32(parent), _u32(child), _u32(matrix)
    ln = None if lengths is None else _f64(lengths)
    nodes = inst.tips + inst.p.contents.clv_buffers if node_count is None else node_count
    S, R, E = inst.p.contents.states, inst.p.contents.rate_cats, len(pa)
    h = Histories()
    h.out = np.full((replicates, nodes, inst.N), fill, dtype=np.uint8) if want_out else None
    h.component = np.full((replicates, inst.N), fill, dtype=np.uint8) if want_component else None
    h.counts = np.full((replicates, E, S, S), fill, dtype=np.uint64)
    h.units = np.full((replicates, E, R, S), fill, dtype=np.uint64)
    h.changes = np.full((replicates, E, inst.N), fill, dtype=np.uint8) if flags & PLLHIP_HIST_SITES else None
    h.dropped_edges = np.full((replicates, E), fill, dtype=np.uint64)
    prm = _ancs_params(seed, replicates, first_replicate, flags, alphabet)
    fidx = inst.params if freqs_indices is None else _u32(freqs_indices)
    pidx = inst.params if params_indices is None else _u32(params_indices)
    dropped = C.c_ulonglong(0)
    ubyte_p, ull_p = C.POINTER(C.c_ubyte), C.POINTER(C.c_ulonglong)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    rn, rs, on, os_ = root_edge
    if not inst.L.pllhip_sample_histories_edges(inst.p, C.byref(prm), rn, rs, on, os_, E, ptr(pa, c_uint_p),
                                                ptr(ch, c_uint_p), ptr(mi, c_uint_p), ptr(fidx, c_uint_p), nodes,
                                                ptr(pidx, c_uint_p), ptr(ln, c_double_p), ptr(h.out, ubyte_p),
                                                ptr(h.component, ubyte_p), C.byref(dropped), ptr(h.counts, ull_p),
                                                ptr(h.units, ull_p), ptr(h.changes, ubyte_p), ptr(h.dropped_edges, ull_p)):
        err = RuntimeError(inst.lib.errmsg)
        err.partial = h
        raise err
    h.dropped = dropped.value
    return h


def sample_histories_utree(inst, root, seed, replicates=1, first_replicate=0, flags=0, alphabet=None):
    """pllhip_sample_histories_utree from `root` (a POINTER(UNode) at an inner node) -> Histories with edge_matrix"""
    nodes = inst.tips + inst.p.contents.clv_buffers
    S, R = inst.p.contents.states, inst.p.contents.rate_cats
    h = Histories()
    h.out = np.zeros((replicates, nodes, inst.N), dtype=np.uint8)
    h.component = np.zeros((replicates, inst.N), dtype=np.uint8)
    counts = np.zeros((replicates, nodes, S, S), dtype=np.uint64)          # (a tree has fewer edges than vectors)
    units = np.zeros((replicates, nodes, R, S), dtype=np.uint64)
    changes = np.zeros((replicates, nodes, inst.N), dtype=np.uint8) if flags & PLLHIP_HIST_SITES else None
    dropped_edges = np.zeros((replicates, nodes), dtype=np.uint64)
    edge_matrix, E = np.zeros(nodes, dtype=np.uint32), C.c_uint(0)
    prm = _ancs_params(seed, replicates, first_replicate, flags, alphabet)
    dropped = C.c_ulonglong(0)
    ubyte_p, ull_p = C.POINTER(C.c_ubyte), C.POINTER(C.c_ulonglong)
    if not inst.L.pllhip_sample_histories_utree(inst.p, C.byref(prm), root, inst.params_p, inst.params_p,
                                                h.out.ctypes.data_as(ubyte_p), h.component.ctypes.data_as(ubyte_p),
                                                C.byref(dropped), counts.ctypes.data_as(ull_p), units.ctypes.data_as(ull_p),
                                                None if changes is None else changes.ctypes.data_as(ubyte_p),
                                                dropped_edges.ctypes.data_as(ull_p), C.byref(E),
                                                edge_matrix.ctypes.data_as(c_uint_p)):
        raise RuntimeError(inst.lib.errmsg)
    E = E.value
    # the library fills [replicates][E][...] densely from the start of each array
    h.counts = counts.reshape(-1)[:replicates * E * S * S].reshape(replicates, E, S, S).copy()
    h.units = units.reshape(-1)[:replicates * E * R * S].reshape(replicates, E, R, S).copy()
    h.changes = None if changes is None else changes.reshape(-1)[:replicates * E * inst.N].reshape(replicates, E, inst.N).copy()
    h.dropped_edges = dropped_edges.reshape(-1)[:replicates * E].reshape(replicates, E).copy()
    h.edge_matrix, h.dropped = edge_matrix[:E].copy(), dropped.value
    return h


def history_last_times(lib):
    """(table_ms, walk_ms, history_ms, copy_ms) of this thread's last pllhip_sample_histories_edges"""
    t = [C.c_double(0.0) for _ in range(4)]
    lib.lib.pllhip_history_last_times(*[C.byref(x) for x in t])
    return tuple(x.value for x in t)


def state_charmap(nstates):
    """a 256-entry char -> mask map where byte value 48+i ('0'+i) means state i and
    '-' means every state (so uint8 state arrays + 48 are valid sequences)"""
    m = np.zeros(256, dtype=np.uint64)
    for i in range(nstates):
        m[48 + i] = np.uint64(1) << np.uint64(i)
    m[ord("-")] = (np.uint64(1) << np.uint64(nstates)) - np.uint64(1) if nstates < 64 else _M64
    return m


class SprParams(C.Structure):
    """pllhip_spr_params_t, include/pllhip_eval.h"""
    _fields_ = [("radius_min", C.c_uint), ("radius_max", C.c_uint), ("ntopol_keep", C.c_uint),
                ("thorough", C.c_int), ("bl_min", C.c_double), ("bl_max", C.c_double),
                ("smoothings", C.c_int), ("epsilon", C.c_double), ("subtree_cutoff", C.c_double),
                ("lh_epsilon_brlen_triplet", C.c_double)]


class SprCutoff(C.Structure):
    _fields_ = [("lh_start", C.c_double), ("lh_cutoff", C.c_double), ("lh_dec_sum", C.c_double),
                ("lh_dec_count", C.c_int)]


SPR_LOG_MAX = 256


class SprStats(C.Structure):
    _fields_ = [("prunings", C.c_ulong), ("insertions", C.c_ulong), ("moves_applied", C.c_ulong),
                ("rescored", C.c_ulong), ("lnl_start", C.c_double), ("lnl_scan", C.c_double),
                ("lnl_final", C.c_double), ("log_count", C.c_uint),
                ("log_prune", C.c_uint * SPR_LOG_MAX), ("log_regraft", C.c_uint * SPR_LOG_MAX)]


class Evaluation:
    """pll_utree_t + partitions + pllhip_eval driver (include/pllhip_eval.h).

    The tree comes from a newick string; tips are matched to alignment rows by
    their labels "t<k>" (the parser numbers tips in order of appearance)."""

    def __init__(self, lib, newick, flags=0, nparts=1):
        self.lib, self.L = lib, lib.lib
        self.utree = self.L.pll_utree_parse_newick_string(newick.encode())
        if not self.utree:
            raise RuntimeError(lib.errmsg)
        tr = self.utree.contents
        self.ntips = tr.tip_count
        # row k of an alignment belongs to the tip labelled t<k>
        self.tip_clv = {}
        for i in range(self.ntips):
            nd = tr.nodes[i].contents
            self.tip_clv[int(nd.label.decode()[1:])] = nd.clv_index
        self.ev = self.L.pllhip_eval_create(self.utree, nparts, flags)
        if not self.ev:
            raise RuntimeError(lib.errmsg)
        self.parts = []

    def add_partition(self, index, states, nsites, rate_cats, codes, subst, freqs, alpha, coded=True,
                      attributes=0):
        inst = Instance(self.lib, self.ntips, states, nsites, rate_cats,
                        attributes=(PLL_ATTRIB_PATTERN_TIP if coded else 0) | attributes)
        rates = self.lib.gamma_cats(alpha, rate_cats) if rate_cats > 1 else np.ones(1)
        inst.set_model(subst, freqs, rates)
        cmap = state_charmap(states)
        for k in range(self.ntips):
            inst.set_tip_states(self.tip_clv[k], cmap, (codes[k] + 48).tobytes())
        if not self.L.pllhip_eval_set_partition(self.ev, index, inst.p, inst.params_p):
            raise RuntimeError(self.lib.errmsg)
        self.parts.append(inst)
        return inst

    def add_remote_partition(self, index):
        """a partition another worker owns: a NULL slot (src/tree/treeinfo.c:1024-1031)"""
        if not self.L.pllhip_eval_set_partition(self.ev, index, None, None):
            raise RuntimeError(self.lib.errmsg)

    def set_parallel_context(self, cb, ctx=None):
        """cb: a REDUCE_CB instance (kept alive here) or a raw function pointer"""
        self._cb = cb
        self.L.pllhip_eval_set_parallel_context(self.ev, ctx, C.cast(cb, C.c_void_p))

    def attach_comm(self, comm=None):
        """deferred results (device-side reduce); product library only"""
        if not self.L.pllhip_eval_attach_comm(self.ev, comm):
            raise RuntimeError(self.lib.errmsg)

    def records(self):
        """every node record of the tree (pll_unode_t pointers)"""
        tr = self.utree.contents
        for i in range(tr.tip_count + tr.inner_count):
            n = tr.nodes[i]
            s_ = n
            while True:
                yield s_
                if not s_.contents.next:
                    break
                s_ = s_.contents.next
                if C.addressof(s_.contents) == C.addressof(n.contents):
                    break

    def set_linkage(self, linkage, scalers=None):
        """0 linked, 1 scaled (per-partition scalers), 2 unlinked (per-partition lengths =
        tree length x scalers[p] to start with)"""
        if not self.L.pllhip_eval_set_brlen_linkage(self.ev, linkage):
            raise RuntimeError(self.lib.errmsg)
        for p, sc in enumerate(scalers or []):
            if linkage == 1:
                if not self.L.pllhip_eval_set_brlen_scaler(self.ev, p, sc):
                    raise RuntimeError(self.lib.errmsg)
            elif linkage == 2:
                for rec in self.records():
                    if not self.L.pllhip_eval_set_partition_branch_length(self.ev, p, rec, rec.contents.length * sc):
                        raise RuntimeError(self.lib.errmsg)

    def partition_tree_length(self, p):
        tot = 0.0
        for rec in self.records():
            tot += self.L.pllhip_eval_get_partition_branch_length(self.ev, p, rec) * \
                self.L.pllhip_eval_get_brlen_scaler(self.ev, p) / 2
        return tot

    def newton_iterations(self):
        return self.L.pllhip_eval_newton_iterations(self.ev)

    def root_edge(self):
        """(clv, scaler, back clv, back scaler, pmatrix) of the edge the lnL is computed at"""
        r = self.L.pllhip_eval_root(self.ev).contents
        b = r.back.contents
        return r.clv_index, r.scaler_index, b.clv_index, b.scaler_index, r.pmatrix_index

    def persite_lnl(self, index=0):
        """per-site lnL of partition `index` at the root edge (CLVs must be valid: call loglh first)"""
        pc_, psc, cc, csc, m = self.root_edge()
        return self.parts[index].edge_lnl(pc_, psc, cc, csc, m, persite=True)

    def set_transient(self, mode):
        """0 off, 1 every full evaluation, 2 a full evaluation that directly follows one (include/pllhip_eval.h)"""
        self.L.pllhip_eval_set_transient(self.ev, int(mode))

    def loglh(self, incremental=False):
        v = self.L.pllhip_eval_loglh(self.ev, 1 if incremental else 0)
        if v != v:
            raise RuntimeError(self.lib.errmsg)
        return v

    def compute_ancestral(self, flags=0):
        """pllhip_eval_compute_ancestral -> Ancestral (numpy copies; the C object is destroyed here)"""
        self.lib.errno = 0
        ptr = self.L.pllhip_eval_compute_ancestral(self.ev, flags)
        if not ptr:
            raise RuntimeError(f"[{self.lib.errno}] {self.lib.errmsg}")
        try:
            a, out = ptr.contents, Ancestral()
            nn, npart = a.node_count, a.partition_count
            recs = [C.cast(a.nodes[i], C.POINTER(UNode)).contents for i in range(nn)]
            out.node_clv = np.array([r.clv_index for r in recs], dtype=np.uint32)
            out.node_index = np.array([r.node_index for r in recs], dtype=np.uint32)
            out.partition_indices = np.array([a.partition_indices[k] for k in range(npart)], dtype=np.uint32)
            out.site_offset = np.array([a.site_offset[k] for k in range(npart + 1)], dtype=np.int64)
            out.prob_offset = np.array([a.prob_offset[k] for k in range(npart + 1)], dtype=np.int64)
            ns, npr = int(out.site_offset[-1]), int(out.prob_offset[-1])
            out.states = np.zeros((nn, ns), dtype=np.uint8)
            out.state_probs = np.zeros((nn, ns))
            out.probs = np.zeros((nn, npr)) if a.probs else None
            for i in range(nn):
                if ns:
                    out.states[i] = np.ctypeslib.as_array(a.states[i], shape=(ns,))
                    out.state_probs[i] = np.ctypeslib.as_array(a.state_probs[i], shape=(ns,))
                if a.probs and npr:
                    out.probs[i] = np.ctypeslib.as_array(a.probs[i], shape=(npr,))
            return out
        finally:
            self.L.pllhip_eval_destroy_ancestral(ptr)

    def site_rates(self, flags=0):
        """pllhip_eval_site_rates -> [SitePosteriors per local partition] (numpy copies)"""
        self.lib.errno = 0
        arr = self.L.pllhip_eval_site_rates(self.ev, flags)
        if not arr:
            raise RuntimeError(f"[{self.lib.errno}] {self.lib.errmsg}")
        try:
            out, k = [], 0
            while arr[k]:
                out.append(SitePosteriors(arr[k].contents))
                k += 1
            return out
        finally:
            self.L.pllhip_eval_destroy_site_rates(arr)

    def sample_ancestral(self, seed, replicates=1, first_replicate=0, flags=0, alphabet=None):
        """pllhip_eval_sample_ancestral -> [SampledAncestral per local partition] (numpy copies)"""
        self.lib.errno = 0
        prm = _ancs_params(seed, replicates, first_replicate, flags, alphabet)
        ptr = self.L.pllhip_eval_sample_ancestral(self.ev, C.byref(prm))
        if not ptr:
            raise RuntimeError(f"[{self.lib.errno}] {self.lib.errmsg}")
        try:
            res, out = ptr.contents, []
            rows, reps = res.node_count, res.replicates
            for k in range(res.partition_count):
                o, N = SampledAncestral(), res.sites[k]
                o.partition = res.partition_indices[k]
                o.clv_index = np.array([res.clv_index[i] for i in range(rows)], dtype=np.uint32)
                o.out = np.ctypeslib.as_array(res.out[k], shape=(reps, rows, N)).copy() if N else np.zeros((reps, rows, 0), np.uint8)
                o.component = np.ctypeslib.as_array(res.component[k], shape=(reps, N)).copy() if N else np.zeros((reps, 0), np.uint8)
                o.dropped = res.dropped[k]
                out.append(o)
            return out
        finally:
            self.L.pllhip_eval_destroy_sampled_ancestral(ptr)

    def sample_histories(self, seed, replicates=1, first_replicate=0, flags=0, alphabet=None):
        """pllhip_eval_sample_histories -> [SampledHistories per local partition] (numpy copies)"""
        self.lib.errno = 0
        prm = _ancs_params(seed, replicates, first_replicate, flags, alphabet)
        ptr = self.L.pllhip_eval_sample_histories(self.ev, C.byref(prm))
        if not ptr:
            raise RuntimeError(f"[{self.lib.errno}] {self.lib.errmsg}")
        try:
            res, out = ptr.contents, []
            rows, reps, E = res.node_count, res.replicates, res.branch_count

            def arr(p, shape, dtype):
                n = int(np.prod(shape))
                return np.ctypeslib.as_array(p, shape=(n,)).reshape(shape).copy() if n else np.zeros(shape, dtype)

            for k in range(res.partition_count):
                o, N, S, R = SampledHistories(), res.sites[k], res.states[k], res.cats[k]
                o.partition = res.partition_indices[k]
                o.clv_index = np.array([res.clv_index[i] for i in range(rows)], dtype=np.uint32)
                o.out = arr(res.out[k], (reps, rows, N), np.uint8)
                o.component = arr(res.component[k], (reps, N), np.uint8)
                o.dropped = res.dropped[k]
                o.counts = arr(res.counts[k], (reps, E, S, S), np.uint64)
                o.units = arr(res.units[k], (reps, E, R, S), np.uint64)
                o.dwell = arr(res.dwell[k], (reps, E, S), np.float64)
                o.total = arr(res.total[k], (reps, E), np.float64)
                o.dropped_edges = arr(res.dropped_edges[k], (reps, E), np.uint64)
                o.changes = arr(res.changes[k], (reps, E, N), np.uint8) if res.changes else None
                out.append(o)
            return out
        finally:
            self.L.pllhip_eval_destroy_sampled_histories(ptr)

    def substitution_map(self, flags=0):
        """pllhip_eval_substitution_map -> [[BranchSubst per branch, by pmatrix_index] per local partition]"""
        self.lib.errno = 0
        ptr = self.L.pllhip_eval_substitution_map(self.ev, flags)
        if not ptr:
            raise RuntimeError(f"[{self.lib.errno}] {self.lib.errmsg}")
        try:
            res, out = ptr.contents, []
            for k in range(res.partition_count):
                rows = []
                for m in range(res.branch_count):
                    b, o = res.branches[k][m], BranchSubst()
                    node = C.cast(b.node, C.POINTER(UNode)).contents
                    S, R, N = b.states, b.cats, b.sites
                    o.parent, o.child, o.matrix = node.clv_index, node.back.contents.clv_index, node.pmatrix_index
                    o.parent_scaler, o.child_scaler = node.scaler_index, node.back.contents.scaler_index
                    o.length = node.length
                    o.pairs = np.ctypeslib.as_array(b.pairs, shape=(R, S, S)).copy()
                    o.counts = np.ctypeslib.as_array(b.counts, shape=(S, S)).copy()
                    o.dwell = np.ctypeslib.as_array(b.dwell, shape=(S,)).copy()
                    o.differ = (np.ctypeslib.as_array(b.differ, shape=(N,)).copy() if N else np.zeros(0)) if b.differ else None
                    o.total, o.posterior_weight, o.dropped = b.total, b.posterior_weight, b.dropped
                    rows.append(o)
                out.append(rows)
            return out
        finally:
            self.L.pllhip_eval_destroy_substitution_map(ptr)

    def optimize_rate_weights(self, partition=0, epsilon=1e-3, max_iterations=100):
        """pllhip_eval_optimize_rate_weights -> (lnL of the driver afterwards, EmFit of the trail)"""
        self.lib.errno = 0
        v = self.L.pllhip_eval_optimize_rate_weights(self.ev, partition, epsilon, max_iterations)
        if v != v:
            raise RuntimeError(f"[{self.lib.errno}] {self.lib.errmsg}")
        cats = self.parts[partition].R
        tw, tl = np.zeros((SITECAT_TRAIL_MAX, cats)), np.zeros(SITECAT_TRAIL_MAX)
        n = self.L.pllhip_eval_rate_weights_trail(self.ev, tw.ctypes.data_as(c_double_p), tl.ctypes.data_as(c_double_p))
        fit = EmFit()
        fit.trail_weights, fit.trail_loglh = tw[:n].copy(), tl[:n].copy()
        p = self.parts[partition].p.contents
        fit.weights = np.array([p.rate_weights[r] for r in range(cats)])
        fit.loglh, fit.iterations = (tl[n - 1] if n else float("nan")), n - 1
        return v, fit

    def optimize_branches(self, bl_min=1e-4, bl_max=10.0, eps=0.01, iters=8, radius=-1):
        self.lib.errno = 0
        v = self.L.pllhip_eval_optimize_branches(self.ev, bl_min, bl_max, eps, iters, radius)
        if v == 0.0 or self.lib.errno:
            raise RuntimeError(f"[{self.lib.errno}] {self.lib.errmsg}")
        return -v

    def spr_round(self, radius_min=1, radius_max=5, ntopol_keep=5, thorough=False, bl_min=1e-4,
                  bl_max=10.0, smoothings=8, epsilon=0.1, subtree_cutoff=1.0, triplet_epsilon=0.1,
                  cutoff=None):
        """one SPR round; returns (lnL, SprStats); `cutoff` (SprCutoff) is carried between rounds"""
        prm = SprParams(radius_min, radius_max, ntopol_keep, int(thorough), bl_min, bl_max, smoothings,
                        epsilon, subtree_cutoff, triplet_epsilon)
        st = SprStats()
        self.lib.errno = 0
        v = self.L.pllhip_eval_spr_round(self.ev, C.byref(prm), C.byref(cutoff) if cutoff is not None else None,
                                         C.byref(st))
        if v == 0.0:
            raise RuntimeError(f"[{self.lib.errno}] {self.lib.errmsg}")
        return v, st

    def newick(self):
        root = self.L.pllhip_eval_root(self.ev)
        ptr = self.L.pll_utree_export_newick(root, None)
        text = C.string_at(ptr).decode()
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        libc.free(ptr)
        return text

    def counters(self):
        return (self.L.pllhip_eval_ops(self.ev), self.L.pllhip_eval_pmatrix_updates(self.ev),
                self.L.pllhip_eval_derivative_calls(self.ev))

    def close(self):
        if self.ev:
            self.L.pllhip_eval_destroy(self.ev)
            self.ev = None
        for p in self.parts:
            p.close()
        self.parts = []
        if self.utree:
            self.L.pll_utree_destroy(self.utree, None)
            self.utree = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


CONFIGS = {
    # name: (states, rate_cats, taxa, sites)   BASELINE.json configs
    "c1": (4, 1, 10, 1000),
    "c2": (4, 4, 100, 1_000_000),
    "c3": (20, 4, 200, 1_000_000),
    "c4": (20, 4, 100, 1_000_000),     # site count split 25/25/12.5/12.5 % over 2 DNA + 2 protein partitions
    "c5": (61, 4, 50, 200_000),
}


def mixture_component(subst, freqs, m):
    """model of mixture component m > 0: the base model's exchangeabilities and frequencies under
    seeded log-normal / Gamma noise (component 0 is the base model itself)"""
    subst, freqs = np.asarray(subst, dtype=float), np.asarray(freqs, dtype=float)
    if m == 0:
        return subst, freqs
    u = uniform01(9000 + 17 * m, 2 * len(subst))
    z = np.sqrt(-2.0 * np.log(np.maximum(u[0::2], 1e-300))) * np.cos(2 * np.pi * u[1::2])
    sub = subst * np.exp(0.4 * z)
    g = freqs * (0.5 + uniform01(9500 + 17 * m, len(freqs)))
    return sub, g / g.sum()


def build_instance(lib, states, rate_cats, ntips, nsites, coded=True, scalers=True, alpha=None,
                   seed_shift=0, tree=None, pinv=0.0, attributes=0, mixture=None, mixture_pinv=None, codes=None):
    """partition + tree + model + tips for one synthetic configuration.
    mixture: per-rate-category rate-matrix indices (e.g. [0, 1, 0, 1]): the partition gets
    max(mixture) + 1 rate matrices, each with a model of its own (mixture_component) and, with
    mixture_pinv, its own proportion of invariant sites."""
    tree = tree or Tree(ntips, 42 + seed_shift, 43 + seed_shift)
    nrm = 1 if mixture is None else int(max(mixture)) + 1
    inst = Instance(lib, ntips, states, nsites, rate_cats,
                    attributes=(PLL_ATTRIB_PATTERN_TIP if coded else 0) | attributes, scalers=scalers,
                    rate_matrices=nrm)
    if states == 4:
        subst, freqs, a = DNA_GTR_RATES, DNA_FREQS, 0.841
    elif states == 20:
        (subst, freqs), a = protein_model(), 0.5
    elif states == 61:
        (subst, freqs), a = codon_model(), 0.5
    else:
        ns = states * (states - 1) // 2
        subst = 0.5 + uniform01(146 + states, ns)
        f = 0.5 + uniform01(147 + states, states)
        freqs, a = f / f.sum(), 0.7
    alpha = a if alpha is None else alpha
    rates = lib.gamma_cats(alpha, rate_cats) if rate_cats > 1 else np.ones(1)
    inst.set_model(subst, freqs, rates)
    if mixture is not None:
        assert len(mixture) == rate_cats
        for m in range(1, nrm):
            inst.set_model(*mixture_component(subst, freqs, m), rates, idx=m)
        inst.set_params_indices(mixture)
    cmap = state_charmap(states)
    if codes is None:
        codes = random_codes(ntips, nsites, states, 44 + seed_shift)
    for t in range(ntips):
        inst.set_tip_states(t, cmap, (codes[t] + 48).tobytes())
    if pinv > 0:
        inst.set_pinv(pinv)
    if mixture_pinv is not None:
        if not inst.L.pll_update_invariant_sites(inst.p):
            raise RuntimeError(lib.errmsg)
        for m, v in enumerate(mixture_pinv):
            inst.set_pinv(v, idx=m)
    inst.tree = tree
    inst.codes = codes
    return inst


def newton_branch_multi(lib, insts, psc, csc, sumtables, scalers, start, bl_min, bl_max, tolerance, max_newton):
    """pllhip_newton_branch_multi over `insts` (their own sumtables, optional branch-length scalers):
    (length, iterations, trail) or raises NewtonError with the library's message"""
    n = len(insts)
    parts = (C.POINTER(Partition) * n)(*[i.p for i in insts])
    params = (c_uint_p * n)(*[i.params_p for i in insts])
    sts = (c_double_p * n)(*[C.cast(s_, c_double_p) for s_ in sumtables])
    sc = _f64(scalers) if scalers is not None else None
    length, its = C.c_double(float("nan")), C.c_uint(0)
    trail = np.zeros(96)
    lib.errno = 0
    ok = lib.lib.pllhip_newton_branch_multi(parts, n, psc, csc, params, sts, sc.ctypes.data_as(c_double_p) if sc is not None else None,
                                            start, bl_min, bl_max, tolerance, max_newton, C.byref(length), C.byref(its),
                                            trail.ctypes.data_as(c_double_p))
    if not ok:
        raise NewtonError(lib, length.value, its.value, trail)
    return length.value, its.value, trail[:its.value]


def update_partials_batch(lib, insts, ops, count=None):
    """pllhip_update_partials_batch over `insts` (None = a partition another worker owns)"""
    if not isinstance(ops, C.Array):
        count = len(ops)
        ops = Instance.make_ops(ops)
    arr = (C.POINTER(Partition) * len(insts))(*[i.p if i is not None else None for i in insts])
    lib.errno = 0
    if not lib.lib.pllhip_update_partials_batch(arr, len(insts), ops, len(ops) if count is None else count):
        raise RuntimeError(lib.errmsg)


def full_traversal(inst, one_by_one_pmatrices=False):
    """the W1 workload: all P-matrices, n-2 partial ops, one edge lnL
    (call pattern of treeinfo_compute_loglh, src/tree/treeinfo.c:946-1079)"""
    t = inst.tree
    key = (id(t), t.root_matrix)
    if getattr(inst, "_trav_key", None) != key:      # C arrays built once per (tree, root)
        inst._trav_key = key
        inst._trav_mi = _u32(np.arange(t.nedges))
        inst._trav_ops = inst.make_ops(t.ops_with_scalers(inst.nscalers > 0))
        inst._trav_nops = len(t.ops)
    if one_by_one_pmatrices:
        # one call per branch, as treeinfo issues them (src/tree/treeinfo.c:845-865);
        # the argument pointers are prepared once so that the loop is just the calls
        if getattr(inst, "_trav_ptrs", None) is None or inst._trav_ptrs[0] != key:
            bl = inst._trav_bl = _f64(t.brlens)
            inst._trav_ptrs = (key, [(C.cast(inst._trav_mi.ctypes.data + 4 * k, c_uint_p),
                                      C.cast(bl.ctypes.data + 8 * k, c_double_p))
                                     for k in range(t.nedges)])
        inst._trav_bl[:] = t.brlens
        fn, p, pp = inst.L.pll_update_prob_matrices, inst.p, inst.params_p
        for mi_p, bl_p in inst._trav_ptrs[1]:
            if not fn(p, pp, mi_p, bl_p, 1):
                raise RuntimeError(inst.lib.errmsg)
    else:
        bl = _f64(t.brlens)
        if not inst.L.pll_update_prob_matrices(inst.p, inst.params_p,
                                               inst._trav_mi.ctypes.data_as(c_uint_p),
                                               bl.ctypes.data_as(c_double_p), t.nedges):
            raise RuntimeError(inst.lib.errmsg)
    inst.update_partials(inst._trav_ops, inst._trav_nops)
    sa = t.scaler_of(t.root_a) if inst.nscalers else PLL_SCALE_BUFFER_NONE
    sb = t.scaler_of(t.root_b) if inst.nscalers else PLL_SCALE_BUFFER_NONE
    return inst.edge_lnl(t.root_a, sa, t.root_b, sb, t.root_matrix)
