"""desc_amd -- MI355X-native implementation of the DESC projected-gradient hot path
(ColeWyeth/DESC, Algorithms/DESC_PGD.m) behind the reference's call signatures.

The numerical work lives in libdesc_amd.so (hand-written HIP for gfx950, C ABI in
include/desc_amd.h).  Importing the package does not need a GPU; creating a solver
does, and there is no CPU fallback.
"""
from .stepsize import ConstantStepSize, HybridGradient, PiecewiseStepSize  # noqa: F401
from .algorithms import CEMP, CEMP_batch, CEMP_GCW, CEMP_GCW_batch, CEMP_MST_batch, MST_batch, DESC, DESC_batch, DESC_refine_batch, DESC_PGD, DESC_PGD_batch, DESC_init, DESC_init_batch, GCW, GCW_batch, Spectral_batch, linprog_sij, linprog_sij_batch, IRLS_GM, IRLS_GM_batch, IRLS_L12, IRLS_L12_batch, MPLS, MPLS_batch, MST, Rotation_Alignment, Rotation_Alignment_batch, Spectral, ProblemBatch  # noqa: F401
from .models import Nonuniform_Topology, Nonuniform_Topology_batch, Uniform_Topology, Uniform_Topology_batch  # noqa: F401

__all__ = ["DESC", "DESC_PGD", "DESC_PGD_batch", "DESC_init", "DESC_init_batch", "DESC_batch", "DESC_refine_batch", "Spectral_batch", "GCW_batch", "CEMP_batch", "CEMP_GCW_batch", "MST_batch", "CEMP_MST_batch", "MPLS_batch", "linprog_sij", "linprog_sij_batch", "IRLS_GM_batch", "IRLS_L12_batch", "CEMP", "MPLS", "MST", "CEMP_GCW", "IRLS_GM", "IRLS_L12", "Spectral", "GCW", "Rotation_Alignment", "Rotation_Alignment_batch", "ProblemBatch", "ConstantStepSize", "PiecewiseStepSize", "HybridGradient",
           "Uniform_Topology", "Nonuniform_Topology", "Uniform_Topology_batch", "Nonuniform_Topology_batch"]
