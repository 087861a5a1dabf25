"""MI355X-native spectral-clustering core for Spectral Cluster Supertree.

Public API mirrors the reference package (reference: src/sc_supertree/__init__.py:6-9):
``construct_supertree`` and ``load_trees``; ``score_supertree`` (RF distances to the sources, clade
support), ``refine_supertree`` (a hill-climb on the triplet distance) and ``resolve_polytomies`` (the
supertree's polytomies resolved from the sources' triples), ``source_distances`` (the sources against one another)
, ``source_coverage`` (which taxa the sources ever show together) and ``source_internode_distances`` (the sources'
average internode distance matrix) are this package's own.
"""

from spectralclustersupertree_amd.load import load_trees
from spectralclustersupertree_amd.scs import construct_supertree
from spectralclustersupertree_amd.score import (InternodeDistances, SourceCoverage, SourceDistances, SupertreeScore,
                                                score_supertree, source_coverage, source_distances,
                                                source_internode_distances)
from spectralclustersupertree_amd.refine import RefineResult, apply_moves, refine_supertree  # noqa: I001
from spectralclustersupertree_amd.resolve import ResolveResult, resolve_polytomies  # noqa: I001

__all__ = ["InternodeDistances", "RefineResult", "ResolveResult", "SourceCoverage", "SourceDistances", "SupertreeScore", "apply_moves",
           "construct_supertree", "load_trees", "refine_supertree", "resolve_polytomies", "score_supertree",
           "source_coverage", "source_distances", "source_internode_distances"]
__version__ = "0.1.0"
