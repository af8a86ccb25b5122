"""singlet_amd: MI355X (gfx950) engine for singlet's ALS hot path
(c_nmf / c_ard_nmf / c_project_model / c_gcnmf / c_LKNN / c_SNN / spatial_graph / rowwise_compress_* of src/singlet.cpp) behind a C ABI
(include/singlet_hip.h), plus the Python mirror of the R interface above it."""
from .sparse import dgCMatrix, as_dgCMatrix  # noqa: F401
from .context import Context, Multi, comm_unique_id, comm_available, device_count, split_cells_by_nnz, graph_halo_plan, LEVELS16, SYNTH_SEED  # noqa: F401
from .api import (c_nmf, c_ard_nmf, c_linked_nmf, c_gcnmf, run_gcnmf, c_nmf_dense, c_nmf_sparse_list, c_ard_nmf_dense, c_ard_nmf_sparse_list, c_project_model, Rcpp_predict, run_nmf, ard_nmf, cross_validate_nmf,  # noqa: F401
                  GetBestRank, project_model, CVData, PreprocessData, weight_by_split, call_times, c_LKNN, c_SNN,
                  find_local_neighbors, rescale_spatial, spatial_graph,
                  rowwise_compress_sparse, rowwise_compress_dense, RasterizeRowwise, RasterMatrix, subset, RunNMF,
                  group_means, run_linked_nmf, RunLNMF, MetadataSummary, GetSharedFactors, GetUniqueFactors, evaluate,
                  find_variable_features, knn, knn_recall, find_neighbors, ReferenceIndex, transfer_labels, transfer_values, map_query, c_louvain, op_louvain_sweep,
                  louvain_info, find_clusters, c_markers, find_all_markers, find_markers, fuzzy_simplicial_set, umap_layout,
                  op_umap_epoch, umap_info, find_ab_params, run_umap, fuzzy_query, umap_transform, op_umap_transform_epochs,
                  umap_transform_info, project_umap, UmapModel, c_gsea, read_gmt, run_gsea, check_columns, get_designs, annotate_stats,
                  c_annotate, c_group_moments, get_model_fit, get_model_results, AnnotateNMF, c_signature_scores, signature_parse,
                  score_signatures, doublet_parents, doublet_scores, doublet_threshold, score_doublets, moran_graph_moments, moran_stats,
                  c_moran, c_moran_embedding, moran_rank, find_spatially_variable_features, moran_factors, nhood_stats,
                  c_nhood_enrichment, nhood_enrichment, interaction_matrix, ligrec_stats, c_ligrec, read_interactions, ligrec,
                  cooccur_stats, ripley_stats, c_cooccur, co_occurrence, ripley)
from .native import native, NativeMatrix  # noqa: F401
from ._lib import SingletHipError, LIB_PATH  # noqa: F401

__version__ = "0.1.0"
