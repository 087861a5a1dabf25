"""How well a supertree fits its source trees: Robinson-Foulds terms per source tree and clade support per
supertree node, and on request rooted triplet terms per source tree (section 15), clade
conflict counts (section 16), branch concordance factors (section 17), per-branch triplet support (section 18),
per-taxon triplet support (section 20) and taxon placement support (section 22).
Neither the reference nor ``construct_supertree`` computes them.

For a source tree T with leaf set L(T), clusters are leaf sets and a cluster of a tree on L is nontrivial when
2 <= size < |L|.  C(S|T) = the nontrivial sets C ∩ L(T) over the clades C of the supertree S; C(T) = T's own.

* per source tree: ``n_super = |C(S|T)|``, ``n_source = |C(T)|``, ``shared = |C(S|T) ∩ C(T)|`` and
  ``rf = n_super + n_source - 2 shared`` (zeros for trees of fewer than 3 leaves);
* per node C of S (preorder, ``TreeNode.to_flat`` order, unary nodes included): ``informative`` = the trees
  with 2 <= |C ∩ L(T)| < |L(T)|, ``supported`` = those of them with C ∩ L(T) in C(T).  Tips and the root are 0.

Rooted triplets (``triplets=True``).  With L = L(T), m = |L| and S' = S|L, a triple {a, b, c} ⊆ L is *resolved ab|c*
in a tree when some cluster of that tree holds a and b but not c; when no cluster does this for any pair, the triple
is a *fan*.  Per source tree:

* ``t_source`` = the triples T resolves, ``t_super`` = the triples S' resolves, ``t_shared`` = the triples resolved
  the same way in both;
* ``triplet_distance = t_super + t_source - 2 t_shared``: the triples whose topology differs (resolved differently,
  or resolved in one tree and a fan in the other).  Trees of m < 3 leaves give zeros.

With y over T's non-root nodes, z over S''s, py / pz their parents and I(y, z) = |cl(y) ∩ cl(z)| (clusters restricted
to L): ``t_shared`` = Σ_y Σ_z C(I(y,z), 2) (I(py,pz) - I(y,pz) - I(py,z) + I(y,z)) and ``t_source`` =
Σ_y C(|y|, 2) (|py| - |y|), ``t_super`` likewise over S'.  A shared triple ab|c is counted once, at the children of
the two LCAs of a, b, c that hold a and b; the second factor counts the c in (cl(py) ∖ cl(y)) ∩ (cl(pz) ∖ cl(z)).

Clade conflicts (``conflicts=True``).  Two sets A and B *conflict* when A ∩ B ≠ ∅, A ⊄ B and B ⊄ A; a set conflicts
with a tree when it conflicts with one of the tree's clusters.  A cluster the tree displays never conflicts with it,
and a fully resolved tree conflicts with every set it does not display.  With L = L(T) and S' = S|L:

* per source tree: ``n_super_conflict`` = the clusters of C(S|T) that conflict with T, ``n_source_conflict`` = the
  clusters of C(T) that conflict with S' (zeros for trees of fewer than 3 leaves);
* per node C of S: ``conflicting`` = the trees for which C ∩ L(T) is nontrivial and conflicts with T.  So
  ``supported + conflicting <= informative``, and ``informative - supported - conflicting`` counts the sources that
  are compatible with C but do not resolve it (a polytomy there, say): no evidence against C.

Branch concordance (``concordance=True``).  A node C of S is a *quartet branch* when it is not the root, has exactly
two children A (the first in preorder) and B, and its parent has exactly two children, C and its sibling D: the branch
above C then has three nearest-neighbour arrangements, AB|D (the supertree's), AD|B and BD|A.  A source tree T on L is
*decisive* for C when A ∩ L, B ∩ L and D ∩ L are all non-empty; a decisive T is *concordant* when (A ∪ B) ∩ L is a
cluster of T, *alt1* when (A ∪ D) ∩ L is, *alt2* when (B ∪ D) ∩ L is (the three sets conflict pairwise, so at most one
holds) and *other* when none is.  These are the gene concordance and discordance factors of IQ-TREE (gCF, gDF1, gDF2,
gDFP) with the source trees as the genes.

* per node C of S: ``decisive``, ``concordant``, ``alt1``, ``alt2`` (zeros where C is not a quartet branch), so
  ``decisive <= informative``, ``concordant <= supported``, ``alt1 + alt2 <= conflicting`` and
  ``other = decisive - concordant - alt1 - alt2 >= 0``;
* per source tree: ``n_decisive`` = the quartet branches it is decisive for, ``n_concordant`` = those it is concordant
  with, ``n_alternative`` = those where it displays alt1 or alt2.

Per-branch triplet support (``branch_triplets=True``): the graded form of the concordance, which is all-or-nothing
per source (one misplaced taxon inside A moves a source to *other*).  For a quartet branch C and a source T on L that is
decisive for it, with A' = A ∩ L, B' = B ∩ L, D' = D ∩ L, each of the |A'| |B'| |D'| triples (a ∈ A', b ∈ B', d ∈ D')
is resolved ab|d by T (concordant), ad|b (alt1), bd|a (alt2) or left a fan.  ASTRAL's local quartet support and
IQ-TREE's sCF are the unrooted relatives.

* per node C of S, summed over the sources: ``bt_total``, ``bt_concordant``, ``bt_alt1``, ``bt_alt2`` (zeros where C
  is not a quartet branch) and ``bt_fan = bt_total - bt_concordant - bt_alt1 - bt_alt2 >= 0``; ``bt_total > 0``
  exactly where ``decisive > 0``, and a source that is concordant (alt1, alt2) at C gives all of its triples there to
  ``bt_concordant`` (``bt_alt1``, ``bt_alt2``);
* per source tree, the same sums over its branches: ``n_bt_total``, ``n_bt_concordant``, ``n_bt_alternative``
  (alt1 + alt2).  A triple of L belongs to at most one branch, so ``n_bt_total <= t_super`` and
  ``n_bt_concordant <= t_shared``.

With y over T's non-root nodes, py the parent and I(y, X) = |cl(y) ∩ X|: ``bt_concordant`` =
Σ_y I(y,A') I(y,B') (I(py,D') - I(y,D')), ``bt_alt1`` with (A', D', B') and ``bt_alt2`` with (B', D', A') in those
places: a triple resolved ab|d has exactly one y with a, b ∈ y and d ∈ py ∖ y.

Per-taxon triplet support (``taxon_triplets=True``): the triplet terms attributed to the taxa of every triple, to name
the misplaced (*rogue*) taxa that lower the support of every clade on their path.  Per supertree tip x (taxon id =
position in ``taxa``, the tips in preorder), summed over the sources T with x ∈ L(T) and m = |L(T)| >= 3:

* ``tx_trees`` = the number of such sources, ``tx_total`` = Σ C(m-1, 2), the triples of L(T) that hold x;
* ``tx_source`` / ``tx_super`` / ``tx_shared`` = those of them T resolves / S' resolves / both resolve alike;
* ``taxon_triplet_distance = tx_super + tx_source - 2 tx_shared``, ``taxon_fit = tx_shared / tx_source`` and
  ``taxon_instability = taxon_triplet_distance / (tx_super + tx_source)`` in [0, 1].

Every triple has three taxa, so Σ_x ``tx_shared`` = 3 Σ_t ``t_shared`` (likewise ``tx_super``, ``tx_source``) and
Σ_x ``tx_total`` = 3 Σ_t C(m, 3).  A shared triple ab|c is counted at one pair (y, z); with I = I(y,z) and J the
second factor of ``t_shared``, every leaf of cl(y) ∩ cl(z) takes (I - 1) J of the pair's triples (as a or b) and
every leaf of (cl(py) ∖ cl(y)) ∩ (cl(pz) ∖ cl(z)) takes C(I, 2) (as c).

Taxon placement support (``placements=[names]`` or ``placements=N``): where a taxon would fit its sources best.  For a
tip x of S and a node v of S (v may be x itself or an ancestor of x), S_{x→v} is S with x pruned and regrafted on the
edge above v.  Its clusters are, for every cluster C of S, (C ∖ {x}) ∪ {x} when C belongs to a strict ancestor of v and
C ∖ {x} otherwise, and the new cluster (cl(v) ∖ {x}) ∪ {x}; empty sets are dropped.  So S_{x→x} has the clusters of S,
and so has S_{x→v} for x's sibling, for x's parent when it has two children, and for every v with cl(v) ∖ {x} = ∅.
Per query taxon x (``pl_taxa``), summed over the sources T with x ∈ L = L(T) and m = |L| >= 3, over the C(m-1, 2)
triples {x, a, b} ⊆ L:

* ``pl_trees`` = ``tx_trees[x]``, ``pl_total`` = ``tx_total[x]``, ``pl_source`` = the triples T resolves;
* ``pl_super[x][v]`` = the triples S_{x→v}|L resolves, ``pl_shared[x][v]`` = those T and S_{x→v}|L resolve alike;
* ``placement_distance = pl_super + pl_source - 2 pl_shared`` per (x, v): the triplet distance x would have there.
  At x's own node the three counts are ``tx_super[x]``, ``tx_source[x]`` and ``tx_shared[x]``.

With every set restricted to L ∖ {x}: the *groups* of x in T are the clusters y with x ∉ y and x ∈ py (the subtrees
hanging off x's root path, leaves included).  T says ab|x when a and b share a group and xa|b when a ∈ y, b ∉ py.  For
a set c, A(c) = Σ_y C(|y ∩ c|, 2); for a child c of an S node with set q, X(c, q) = Σ_y |y ∩ c| (|q ∖ py| - |c ∖ py|),
the pairs a ∈ c, b ∈ q ∖ c with xa|b in T.  Then shared(root) = A(root set) and, for a node v with parent q,
shared(v) = shared(q) + [Σ_{children s of q} A(s) - A(q)] + X(v, q): moving x from the edge above q to the edge above
v loses the pairs ab|x whose LCA is q and gains the pairs xa|b with a below v and b below q.  ``pl_super`` follows the
same recurrence with C(|c|, 2) and |c| (|q| - |c|).  Every term is node-local, so a value is a root-path sum of marks.

Clade placement support (``clade_placements=[nodes or name sets]`` or ``clade_placements=N``): the same question for a
whole subtree.  For a non-root node q of S with leaf set Q and a node v outside its subtree, S_{q→v} is S with the
subtree of q pruned and regrafted on the edge above v: every cluster C outside the subtree becomes (C ∖ Q) ∪ Q when it
belongs to a strict ancestor of v and C ∖ Q otherwise, the clusters inside the subtree stay, and (cl(v) ∖ Q) ∪ Q is
new.  For v inside the subtree S_{q→v} = S.  Per query (``cp_nodes``), summed over the sources T on L with Q' = Q ∩ L
and R = L ∖ Q both non-empty and |L| >= 3, over the *crossing* triples of L (a taxon in Q' and one in R; no other
triple changes when the clade moves):

* ``cp_trees`` = those sources, ``cp_total`` = their crossing triples, ``cp_source`` = those T resolves;
* ``cp_super[q][v]`` = those S_{q→v}|L resolves, ``cp_shared[q][v]`` = those T and S_{q→v}|L resolve alike;
* ``clade_placement_distance = cp_super + cp_source - 2 cp_shared``: the part of the total triplet distance that the
  move can change, so that distance[q][v] - distance[q][q] is what moving the clade to v adds to it.

For a tip q these are the ``pl_*`` of its taxon.

Polytomy support (``polytomies=True`` or ``polytomies=[nodes or name sets]``): what the sources say about grouping the
children c_0 .. c_{k-1} of a node with three or more of them, where every count above is blind.  Per polytomy
(``py_nodes``), over the sources T on L that hold leaves of at least three children (``py_trees``), with
C_i' = cl(c_i) ∩ L, for i < j and l not in {i, j}:

* ``py_total[q][i][j][l]`` = Σ |C_i'| |C_j'| |C_l'|: the triples with a leaf below c_i, c_j and c_l, all fans in S;
* ``py_joint[q][i][j][l]`` = those of them T resolves with the leaves of c_i and c_j together.

Two groups G and H of children put under one new node lower the summed triplet distance by exactly 2 M - N, M and N
the sums of ``py_joint`` and ``py_total`` over i in G, j in H and l in neither (``polytomy_merge_gain``;
``resolve.resolve_polytomies`` builds a whole resolution on it).

Resampled and weighted branch triplet support (``branch_resample=...`` and / or ``tree_weights=...``): the per-branch
triple counts under R rows of non-negative integer tree weights, rs_x[r][u] = Σ_T w[r][T] bt_x(T, u) with bt_x(T, u)
what T alone adds to ``bt_x[u]``.  A tree of weight w counts exactly like w copies of it, so every number stays an
exact int64.  Row 0 is the point estimate (``tree_weights``, all ones by default: then ``rs_total`` = ``bt_total`` and
so on); rows 1 .. R - 1 are replicates, bootstrap or jackknife draws of the sources (``resample_weights``).  A
replicate with rs_total > 0 at a branch is counted once there: for the arrangement whose count is strictly greatest
(``win_concordant``, ``win_alt1``, ``win_alt2``) or as ``win_tie``; ``branch_support`` = win_concordant over the four
together.  Only this pass is weighted; every other count of this module ignores tree weights.

MRP parsimony (``parsimony=True``): the length of the supertree on the Baum-Ragan matrix of its sources, the
criterion matrix-representation-with-parsimony supertrees minimise.  For a source tree T on leaf set L with m = |L| >= 3
and S' = S|L, the characters of T are its nontrivial clusters C(T) (2 <= |C| < m, each once, in the order of the
clusters' first gaps in T's DFS order); character C gives state 1 to the taxa of C, 0 to L - C and "missing" to every
other tip of S.  len(C) is the least number of state changes of that character on S with an all-zero outgroup attached
above the root (rooted coding), polytomies taken as hard; it equals the length on S' with the outgroup.  len(C) >= 1,
len(C) = 1 iff C is a cluster of S', and len(C) <= gmax(C) = min(|C|, m - |C| + 1), the length on a star.  Per source
tree (zeros for trees of fewer than 3 leaves): ``mrp_chars`` = |C(T)| (= ``n_source``), ``mrp_length`` = Σ len,
``mrp_perfect`` = #{len = 1} (= ``shared``), ``mrp_max`` = Σ gmax; ``mrp_extra`` = length - chars,
``consistency_index`` = Σ chars / Σ length, ``retention_index`` = (Σ max - Σ length) / (Σ max - Σ chars).  With
``parsimony_chars=True`` also the length of every single source clade (``mrp_char_length``, ``mrp_char_clusters``,
``worst_source_clades``, ``annotate_source``): a graded form of ``shared`` / ``n_source_conflict``, as the triplet
distance is a graded form of RF.

Every count comes from the HIP kernels behind ``scs_score_supertree``, ``scs_score_triplets``,
``scs_score_conflicts``, ``scs_score_concordance``, ``scs_score_branch_triplets``, ``scs_score_branch_resample``,
``scs_score_taxon_triplets``, ``scs_score_placements``, ``scs_score_clade_placements``, ``scs_score_polytomies``,
``scs_score_parsimony`` and (for ``refine_supertree``) ``scs_score_clade_moves``; the host only validates and lays out.

``source_distances`` measures the sources against one another instead: the same RF terms between every two source
trees, each pair restricted to the taxa both hold (``scs_score_source_pairs``), and with
``triplets=True`` the rooted-triplet terms of every pair, the graded measure beside RF
(``scs_score_source_pair_triplets``).
``source_coverage`` asks the earlier question, whether the sources overlap enough to determine a tree at all: the
rooted triples of taxa that some source tree holds whole (``scs_score_coverage``).
``source_internode_distances`` gives the sources' answer per pair of taxa: over the trees that hold both, the sum and
the mean of the number of edges between them (``scs_score_internode``) -- the average internode
distance matrix of ASTRID / NJst and of average-consensus supertrees, ready for FastME or any NJ program.
"""

from __future__ import annotations

import time
from contextlib import contextmanager
from dataclasses import dataclass, field, fields, replace

import numpy as np

from spectralclustersupertree_amd.flatten import flatten_trees
from spectralclustersupertree_amd.tree import TreeNode, is_not_completed
from spectralclustersupertree_amd.treearrays import TreeArrays

# trees per device batch; None: sized by the workspace (a test sets a small value to reach the batch loop)
BATCH_TREES: int | None = None
# LDS bytes a workgroup of the per-taxon pair kernel may take; None: the default (a test sets a small value so that
# small trees reach the path through global memory)
TAXON_LDS_BYTES: int | None = None
# the same for the placement pair kernel (a small value: no room for the sums per node and query beside the rows)
PLACEMENT_LDS_BYTES: int | None = None
# and for the clade placement pair kernel
CLADE_PLACEMENT_LDS_BYTES: int | None = None
# and for the polytomy sweep (a small value: no room for the k x k sums beside the rows, or none for the rows)
POLYTOMY_LDS_BYTES: int | None = None


# 64-character words of a source tree one pass of the parsimony fold covers; None: the default, 64 (a test sets a small
# value to reach the pass loop)
PARSIMONY_PASS_WORDS: int | None = None


@dataclass
class SupertreeScore:
    """Scores of ``supertree`` against its sources; int64 arrays."""

    supertree: TreeNode
    n_leaves: np.ndarray  # per source tree
    n_super: np.ndarray
    n_source: np.ndarray
    shared: np.ndarray
    informative: np.ndarray  # per supertree node, preorder
    supported: np.ndarray
    # wall seconds: "prepare" (host: supertree arrays, checks, flattening objects), "tables" (a TreeArrays forest
    # to device tables), "score" (scs_score_supertree: its host layout of the supertree and the kernels),
    # "triplets" (scs_score_triplets, when requested), "conflicts" (scs_score_conflicts, when requested),
    # "concordance" (scs_score_concordance, when requested), "branch_triplets" (scs_score_branch_triplets, when
    # requested), "taxon_triplets" (scs_score_taxon_triplets, when requested), "placements" (scs_score_placements,
    # when requested), "clade_placements" (scs_score_clade_placements, when requested), "polytomies"
    # (scs_score_polytomies, when requested), "branch_resample" (scs_score_branch_resample, when requested),
    # "parsimony" (scs_score_parsimony, when requested)
    timings: dict = field(default_factory=dict)
    # rooted triplet terms per source tree (``triplets=True``; None otherwise)
    t_super: np.ndarray | None = None
    t_source: np.ndarray | None = None
    t_shared: np.ndarray | None = None
    # clade conflicts (``conflicts=True``; None otherwise): per source tree, and per supertree node (preorder)
    n_super_conflict: np.ndarray | None = None
    n_source_conflict: np.ndarray | None = None
    conflicting: np.ndarray | None = None
    # branch concordance (``concordance=True``; None otherwise): per source tree, and per supertree node (preorder)
    n_decisive: np.ndarray | None = None
    n_concordant: np.ndarray | None = None
    n_alternative: np.ndarray | None = None
    decisive: np.ndarray | None = None
    concordant: np.ndarray | None = None
    alt1: np.ndarray | None = None
    alt2: np.ndarray | None = None
    # per-branch triplet support (``branch_triplets=True``; None otherwise): per source tree, and per supertree node
    n_bt_total: np.ndarray | None = None
    n_bt_concordant: np.ndarray | None = None
    n_bt_alternative: np.ndarray | None = None
    bt_total: np.ndarray | None = None
    bt_concordant: np.ndarray | None = None
    bt_alt1: np.ndarray | None = None
    bt_alt2: np.ndarray | None = None
    # per-taxon triplet support (``taxon_triplets=True``; None otherwise): the supertree's tip names in taxon-id order
    # and the counts per taxon
    taxa: list | None = None
    tx_trees: np.ndarray | None = None
    tx_total: np.ndarray | None = None
    tx_super: np.ndarray | None = None
    tx_source: np.ndarray | None = None
    tx_shared: np.ndarray | None = None
    # taxon placement support (``placements=...``; None otherwise): the query taxa (ids into ``taxa``), one entry per
    # query, and queries x supertree nodes (preorder)
    pl_taxa: np.ndarray | None = None
    pl_trees: np.ndarray | None = None
    pl_total: np.ndarray | None = None
    pl_source: np.ndarray | None = None
    pl_super: np.ndarray | None = None
    pl_shared: np.ndarray | None = None
    # clade placement support (``clade_placements=...``; None otherwise): the query nodes (preorder indices), one entry
    # per query, and queries x supertree nodes (preorder)
    cp_nodes: np.ndarray | None = None
    cp_trees: np.ndarray | None = None
    cp_total: np.ndarray | None = None
    cp_source: np.ndarray | None = None
    cp_super: np.ndarray | None = None
    cp_shared: np.ndarray | None = None

    @property
    def rf(self) -> np.ndarray:
        return self.n_super + self.n_source - 2 * self.shared

    @property
    def total_rf(self) -> int:
        """The RF supertree score: the RF distances to the sources, summed."""
        return int(self.rf.sum())

    @property
    def triplet_distance(self) -> np.ndarray:
        """Per source tree: the triples whose topology differs between S|L(T) and T."""
        self._need_triplets()
        return self.t_super + self.t_source - 2 * self.t_shared

    @property
    def total_triplet_distance(self) -> int:
        self._need_triplets()
        return int(self.triplet_distance.sum())

    @property
    def triplet_fit(self) -> float:
        """Σ t_shared / Σ t_source: the share of the sources' resolved triples the supertree resolves alike (NaN when
        no source resolves a triple)."""
        self._need_triplets()
        total = int(self.t_source.sum())
        return float(int(self.t_shared.sum()) / total) if total > 0 else float("nan")

    def _need_triplets(self) -> None:
        if self.t_shared is None:
            msg = "triplet terms were not computed: score_supertree(..., triplets=True)"
            raise ValueError(msg)

    def support(self) -> np.ndarray:
        """``supported / informative`` per node (NaN where no source is informative)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.informative > 0, self.supported / np.maximum(self.informative, 1), np.nan)

    def annotate(self) -> TreeNode:
        """A copy of the supertree whose internal non-root nodes carry ``support`` = supported / informative
        (None where no source is informative) and the same value as their name, so that
        ``get_newick(with_node_names=True)`` writes it."""
        out = self.supertree.copy()
        values = self.support()
        for i, node in enumerate(_preorder(out)):
            if node.is_tip() or i == 0:
                continue
            v = values[i]
            node.support = None if np.isnan(v) else float(v)
            node.name = None if np.isnan(v) else repr(float(v))
        return out

    def annotate_counts(self) -> TreeNode:
        """A copy of the supertree whose internal non-root nodes are named ``supported/conflicting/informative``
        (no name where no source is informative), so that ``get_newick(with_node_names=True)`` writes the counts.
        ``ValueError`` unless the conflicts were computed."""
        if self.conflicting is None:
            msg = "conflict counts were not computed: score_supertree(..., conflicts=True)"
            raise ValueError(msg)
        out = self.supertree.copy()
        for i, node in enumerate(_preorder(out)):
            if node.is_tip() or i == 0:
                continue
            inf = int(self.informative[i])
            node.name = f"{int(self.supported[i])}/{int(self.conflicting[i])}/{inf}" if inf > 0 else None
        return out

    @property
    def quartet_branch(self) -> np.ndarray:
        """Bool mask per node (preorder): not the root, exactly two children, and a parent with exactly two."""
        return quartet_branches(np.asarray(self.supertree.to_flat()[0], dtype=np.int64))

    def _need_concordance(self) -> None:
        if self.decisive is None:
            msg = "concordance counts were not computed: score_supertree(..., concordance=True)"
            raise ValueError(msg)

    @property
    def other(self) -> np.ndarray:
        """Per node: the decisive sources that display none of the three arrangements (IQ-TREE's gDFP count)."""
        self._need_concordance()
        return self.decisive - self.concordant - self.alt1 - self.alt2

    def _percent(self, counts: np.ndarray) -> np.ndarray:
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.decisive > 0, 100.0 * counts / np.maximum(self.decisive, 1), np.nan)

    @property
    def gcf(self) -> np.ndarray:
        """``concordant`` in percent of ``decisive`` (NaN where no source is decisive)."""
        self._need_concordance()
        return self._percent(self.concordant)

    @property
    def gdf1(self) -> np.ndarray:
        """``alt1`` in percent of ``decisive``."""
        self._need_concordance()
        return self._percent(self.alt1)

    @property
    def gdf2(self) -> np.ndarray:
        """``alt2`` in percent of ``decisive``."""
        self._need_concordance()
        return self._percent(self.alt2)

    @property
    def gdfp(self) -> np.ndarray:
        """``other`` in percent of ``decisive``."""
        return self._percent(self.other)

    def annotate_concordance(self) -> TreeNode:
        """A copy of the supertree whose quartet branches are named ``concordant/alt1/alt2/decisive`` and whose other
        internal nodes carry no name, so that ``get_newick(with_node_names=True)`` writes the counts.
        ``ValueError`` unless the concordance was computed."""
        self._need_concordance()
        out = self.supertree.copy()
        mask = self.quartet_branch
        for i, node in enumerate(_preorder(out)):
            if node.is_tip():
                continue
            node.name = (f"{int(self.concordant[i])}/{int(self.alt1[i])}/{int(self.alt2[i])}/{int(self.decisive[i])}"
                         if mask[i] else None)
        return out

    def nni_candidates(self, by: str = "sources", min_support: float | None = None) -> list[dict]:
        """The quartet branches where an alternative arrangement has more sources than the branch itself: one dict
        per branch with ``node`` (preorder index), ``alternative`` (``"alt1"`` or ``"alt2"``, the larger; alt1 on
        a tie), ``decisive``, ``concordant``, ``alt1``, ``alt2`` and ``margin`` = that alternative's count minus
        ``concordant``; largest margin first, then by node.  ``by="triplets"`` compares the per-branch triple
        counts instead (``branch_triplets=True``): the same keys, holding ``bt_total``, ``bt_concordant``,
        ``bt_alt1`` and ``bt_alt2`` (the point estimates ``rs_*`` where only the resampling was computed).
        ``min_support`` (``by="triplets"``, with ``branch_resample=...``): only the branches whose alternative also
        wins in at least that share of the informative replicates, which ``replicate_share`` then holds."""
        if min_support is not None and (by != "triplets" or self.rs_wins is None):
            msg = "min_support needs by='triplets' and replicates: score_supertree(..., branch_resample=N)"
            raise ValueError(msg)
        if by == "sources":
            self._need_concordance()
            dec, con, alt1, alt2 = self.decisive, self.concordant, self.alt1, self.alt2
        elif by == "triplets" and self.bt_total is None and self._rs is not None:
            dec, con, alt1, alt2 = self.rs_total, self.rs_concordant, self.rs_alt1, self.rs_alt2
        elif by == "triplets":
            self._need_branch_triplets()
            dec, con, alt1, alt2 = self.bt_total, self.bt_concordant, self.bt_alt1, self.bt_alt2
        else:
            msg = f"by must be 'sources' or 'triplets', not {by!r}"
            raise ValueError(msg)
        best = np.maximum(alt1, alt2)
        out = []
        for i in np.flatnonzero(best > con):
            out.append({"node": int(i), "alternative": "alt1" if alt1[i] >= alt2[i] else "alt2",
                        "decisive": int(dec[i]), "concordant": int(con[i]),
                        "alt1": int(alt1[i]), "alt2": int(alt2[i]),
                        "margin": int(best[i] - con[i])})
        if min_support is not None:
            wins = self.rs_wins
            informative = sum(wins.values())
            for r in out:
                n = int(informative[r["node"]])
                r["replicate_share"] = int(wins["win_" + r["alternative"]][r["node"]]) / n if n else float("nan")
            out = [r for r in out if r["replicate_share"] >= min_support]
        out.sort(key=lambda r: (-r["margin"], r["node"]))
        return out

    def _need_branch_triplets(self) -> None:
        if self.bt_total is None:
            msg = "branch triplet counts were not computed: score_supertree(..., branch_triplets=True)"
            raise ValueError(msg)

    @property
    def bt_fan(self) -> np.ndarray:
        """Per node: the triples around the branch that their source leaves unresolved."""
        self._need_branch_triplets()
        return self.bt_total - self.bt_concordant - self.bt_alt1 - self.bt_alt2

    def _bt_percent(self, counts: np.ndarray) -> np.ndarray:
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.bt_total > 0, 100.0 * counts / np.maximum(self.bt_total, 1), np.nan)

    @property
    def tcf(self) -> np.ndarray:
        """``bt_concordant`` in percent of ``bt_total`` (NaN where it is zero)."""
        self._need_branch_triplets()
        return self._bt_percent(self.bt_concordant)

    @property
    def tdf1(self) -> np.ndarray:
        """``bt_alt1`` in percent of ``bt_total``."""
        self._need_branch_triplets()
        return self._bt_percent(self.bt_alt1)

    @property
    def tdf2(self) -> np.ndarray:
        """``bt_alt2`` in percent of ``bt_total``."""
        self._need_branch_triplets()
        return self._bt_percent(self.bt_alt2)

    @property
    def tdfu(self) -> np.ndarray:
        """``bt_fan`` in percent of ``bt_total``."""
        return self._bt_percent(self.bt_fan)

    def annotate_branch_triplets(self) -> TreeNode:
        """A copy of the supertree whose branches with ``bt_total > 0`` are named
        ``bt_concordant/bt_alt1/bt_alt2/bt_total`` and whose other internal nodes carry no name, so that
        ``get_newick(with_node_names=True)`` writes the counts.  ``ValueError`` unless they were computed."""
        self._need_branch_triplets()
        out = self.supertree.copy()
        for i, node in enumerate(_preorder(out)):
            if node.is_tip():
                continue
            node.name = (f"{int(self.bt_concordant[i])}/{int(self.bt_alt1[i])}/{int(self.bt_alt2[i])}"
                         f"/{int(self.bt_total[i])}" if self.bt_total[i] > 0 else None)
        return out

    def _need_taxon_triplets(self) -> None:
        if self.tx_shared is None:
            msg = "per-taxon triplet counts were not computed: score_supertree(..., taxon_triplets=True)"
            raise ValueError(msg)

    @property
    def taxon_triplet_distance(self) -> np.ndarray:
        """Per taxon: the triples holding it whose topology differs between S|L(T) and T, over its sources."""
        self._need_taxon_triplets()
        return self.tx_super + self.tx_source - 2 * self.tx_shared

    @property
    def taxon_fit(self) -> np.ndarray:
        """``tx_shared / tx_source`` per taxon (NaN where its sources resolve no triple that holds it)."""
        self._need_taxon_triplets()
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.tx_source > 0, self.tx_shared / np.maximum(self.tx_source, 1), np.nan)

    @property
    def taxon_instability(self) -> np.ndarray:
        """``taxon_triplet_distance / (tx_super + tx_source)`` per taxon, in [0, 1]: 0 when every resolved triple that
        holds the taxon is resolved alike, 1 when none is (NaN where neither tree resolves one)."""
        dist = self.taxon_triplet_distance
        both = self.tx_super + self.tx_source
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(both > 0, dist / np.maximum(both, 1), np.nan)

    def rogue_taxa(self, n: int | None = None, min_trees: int = 1) -> list[dict]:
        """The taxa in at least ``min_trees`` sources (of 3 or more leaves) whose instability is defined: one dict
        per taxon with ``taxon`` (id), ``name``, ``trees``, ``total``, ``super``, ``source``, ``shared``,
        ``distance`` and ``instability``; largest instability first, then larger distance, then id.  The first
        ``n`` when given."""
        inst = self.taxon_instability
        dist = self.taxon_triplet_distance
        out = []
        for x in np.flatnonzero((self.tx_trees >= min_trees) & ~np.isnan(inst)):
            out.append({"taxon": int(x), "name": self.taxa[x], "trees": int(self.tx_trees[x]),
                        "total": int(self.tx_total[x]), "super": int(self.tx_super[x]),
                        "source": int(self.tx_source[x]), "shared": int(self.tx_shared[x]),
                        "distance": int(dist[x]), "instability": float(inst[x])})
        out.sort(key=lambda r: (-r["instability"], -r["distance"], r["taxon"]))
        return out if n is None else out[:n]

    def taxon_table(self) -> str:
        """One TSV row per supertree tip: taxon (id), name, tx_trees, tx_total, tx_super, tx_source, tx_shared,
        triplet_distance.  ``ValueError`` unless the per-taxon counts were computed."""
        dist = self.taxon_triplet_distance
        rows = ["taxon\tname\ttx_trees\ttx_total\ttx_super\ttx_source\ttx_shared\ttriplet_distance"]
        for x, name in enumerate(self.taxa):
            rows.append(f"{x}\t{name}\t{self.tx_trees[x]}\t{self.tx_total[x]}\t{self.tx_super[x]}"
                        f"\t{self.tx_source[x]}\t{self.tx_shared[x]}\t{dist[x]}")
        return "\n".join(rows) + "\n"

    def _need_placements(self) -> None:
        if self.pl_shared is None:
            msg = "placement counts were not computed: score_supertree(..., placements=...)"
            raise ValueError(msg)

    @property
    def placement_distance(self) -> np.ndarray:
        """Queries x nodes: the triplet distance of the query taxon to its sources if it sat on the edge above the
        node."""
        self._need_placements()
        return self.pl_super + self.pl_source[:, None] - 2 * self.pl_shared

    def _tip_nodes(self) -> np.ndarray:
        """Preorder index of every tip, by taxon id."""
        return np.array([i for i, v in enumerate(_preorder(self.supertree)) if v.is_tip()], dtype=np.int64)

    def best_placements(self) -> list[dict]:
        """One dict per query taxon, in query order: ``taxon`` (id), ``name``, ``trees``, ``node`` (the taxon's own
        node, preorder index), ``distance`` (its triplet distance there), ``best_node``, ``best_distance`` and
        ``improvement`` = distance - best_distance >= 0.  The best node has the smallest distance; among equals the
        taxon's own node, else the lowest preorder index."""
        dist = self.placement_distance
        own = self._tip_nodes()
        out = []
        for i, x in enumerate(self.pl_taxa):
            node = int(own[x])
            best, low = _best_node(dist[i], node)
            out.append({"taxon": int(x), "name": self.taxa[x], "trees": int(self.pl_trees[i]), "node": node,
                        "distance": int(dist[i, node]), "best_node": best, "best_distance": low,
                        "improvement": int(dist[i, node]) - low})
        return out

    def placement_table(self) -> str:
        """One TSV row per query taxon: taxon (id), name, trees, node, distance, best_node, best_distance,
        improvement (``best_placements``).  ``ValueError`` unless the placements were computed."""
        rows = ["taxon\tname\ttrees\tnode\tdistance\tbest_node\tbest_distance\timprovement"]
        for r in self.best_placements():
            rows.append(f"{r['taxon']}\t{r['name']}\t{r['trees']}\t{r['node']}\t{r['distance']}\t{r['best_node']}"
                        f"\t{r['best_distance']}\t{r['improvement']}")
        return "\n".join(rows) + "\n"

    def regraft(self, taxon, node: int) -> TreeNode:
        """A copy of the supertree with the tip ``taxon`` (a name, or an id into the tips in preorder) moved onto
        the edge above ``node`` (preorder index in this supertree): S_{x→node} of the module docstring.  The node the
        tip leaves behind is suppressed when it keeps one child; when ``node`` is that node, the tip goes above its
        remaining child.  When ``node`` holds no taxon but the tip itself, the copy is unchanged."""
        out = self.supertree.copy()
        nodes = _preorder(out)
        tips = [v for v in nodes if v.is_tip()]
        if isinstance(taxon, str):
            found = [v for v in tips if v.name == taxon]
            if not found:
                msg = f"taxon {taxon!r} is not in the supertree"
                raise ValueError(msg)
            tip = found[0]
        else:
            if not 0 <= int(taxon) < len(tips):
                msg = f"taxon id {taxon} is not in [0, {len(tips)})"
                raise ValueError(msg)
            tip = tips[int(taxon)]
        if not 0 <= int(node) < len(nodes):
            msg = f"node {node} is not in [0, {len(nodes)})"
            raise ValueError(msg)
        target = nodes[int(node)]
        if all(t is tip for t in target.iter_tips()):
            return out
        return _move_clade(out, tip, target)

    def _need_clade_placements(self) -> None:
        if self.cp_shared is None:
            msg = "clade placement counts were not computed: score_supertree(..., clade_placements=...)"
            raise ValueError(msg)

    @property
    def clade_placement_distance(self) -> np.ndarray:
        """Queries x nodes: the crossing triples whose topology would differ between the sources and the supertree if
        the query clade sat on the edge above the node."""
        self._need_clade_placements()
        return self.cp_super + self.cp_source[:, None] - 2 * self.cp_shared

    def best_clade_placements(self) -> list[dict]:
        """One dict per query clade, in query order: ``node`` (the clade's own node, preorder index), ``tips`` (its
        size), ``trees``, ``distance`` (its value at its own place), ``best_node``, ``best_distance`` and
        ``improvement`` = distance - best_distance >= 0.  The best node has the smallest distance; among equals the
        clade's own node, else the lowest preorder index."""
        dist = self.clade_placement_distance
        lo, hi = _leaf_ranges(np.asarray(self.supertree.to_flat()[0], dtype=np.int64))
        out = []
        for i, q in enumerate(self.cp_nodes):
            node = int(q)
            best, low = _best_node(dist[i], node)
            out.append({"node": node, "tips": int(hi[node] - lo[node] + 1), "trees": int(self.cp_trees[i]),
                        "distance": int(dist[i, node]), "best_node": best, "best_distance": low,
                        "improvement": int(dist[i, node]) - low})
        return out

    def clade_placement_table(self) -> str:
        """One TSV row per query clade: node, tips, trees, distance, best_node, best_distance, improvement
        (``best_clade_placements``).  ``ValueError`` unless the clade placements were computed."""
        rows = ["node\ttips\ttrees\tdistance\tbest_node\tbest_distance\timprovement"]
        for r in self.best_clade_placements():
            rows.append(f"{r['node']}\t{r['tips']}\t{r['trees']}\t{r['distance']}\t{r['best_node']}"
                        f"\t{r['best_distance']}\t{r['improvement']}")
        return "\n".join(rows) + "\n"

    def regraft_clade(self, node: int, target: int) -> TreeNode:
        """A copy of the supertree with the subtree of ``node`` moved onto the edge above ``target`` (preorder indices
        in this supertree): S_{node→target} of the module docstring.  The node the clade leaves behind is suppressed
        when it keeps one child; when ``target`` is that node, the clade goes above its remaining child.  When
        ``target`` holds no taxon outside the clade (a unary ancestor), the copy is unchanged.  ``ValueError`` when
        ``node`` is the root or out of range, or ``target`` is out of range or lies inside the subtree of ``node``."""
        out = self.supertree.copy()
        nodes = _preorder(out)
        if not 1 <= int(node) < len(nodes):
            msg = f"node {node} is the root or not in [1, {len(nodes)})"
            raise ValueError(msg)
        if not 0 <= int(target) < len(nodes):
            msg = f"target {target} is not in [0, {len(nodes)})"
            raise ValueError(msg)
        clade, goal = nodes[int(node)], nodes[int(target)]
        up = goal
        while up is not None:
            if up is clade:
                msg = f"target {target} lies inside the subtree of node {node}"
                raise ValueError(msg)
            up = up.parent
        return _move_clade(out, clade, goal)

    # polytomy support (``polytomies=...``; None otherwise), kept beside the dataclass fields: a dict with the keys
    # of ``_PY_KEYS``, read through the properties below
    _py = None

    @property
    def py_nodes(self) -> np.ndarray | None:
        """The polytomies that were scored (preorder indices), one entry per query."""
        return None if self._py is None else self._py["py_nodes"]

    @property
    def py_degree(self) -> np.ndarray | None:
        """Their numbers of children."""
        return None if self._py is None else self._py["py_degree"]

    @property
    def py_trees(self) -> np.ndarray | None:
        """The sources with three or more of a polytomy's children among their leaves (decisive)."""
        return None if self._py is None else self._py["py_trees"]

    @property
    def py_total(self) -> list | None:
        """Per polytomy a k x k x k array: [i][j][l], i < j, l not in {i, j}: the triples with a leaf below child i,
        one below child j and one below child l, over the decisive sources."""
        return None if self._py is None else self._py["py_total"]

    @property
    def py_joint(self) -> list | None:
        """Those of ``py_total`` the source resolves with the leaves of i and j together."""
        return None if self._py is None else self._py["py_joint"]

    @property
    def py_skipped(self) -> list | None:
        """The polytomies that were not scored: dicts with ``node``, ``degree`` and ``reason``."""
        return None if self._py is None else self._py["py_skipped"]

    def _need_polytomies(self) -> None:
        if self._py is None:
            msg = "polytomy counts were not computed: score_supertree(..., polytomies=True)"
            raise ValueError(msg)

    def polytomy_merge_gain(self, q: int, G, H) -> int:
        """What the summed triplet distance falls by when the children ``G`` and ``H`` (two disjoint, non-empty
        lists of child positions that leave a child out) of polytomy ``q`` (a position in ``py_nodes``) go under one
        new node: 2 M(G, H) - N(G, H)."""
        self._need_polytomies()
        from spectralclustersupertree_amd.resolve import merge_gain

        return merge_gain(self.py_total[q], self.py_joint[q], G, H)

    def polytomy_table(self) -> str:
        """One TSV row per polytomy and pair of its children: node (preorder index), i, j (child positions), tips
        (below the two children), total and joint (the triples with a leaf below each of the two and one below a third
        child, and those the sources resolve with the two together), gain (of merging just that pair)."""
        self._need_polytomies()
        parent = np.asarray(self.supertree.to_flat()[0], dtype=np.int64)
        lo, hi = _leaf_ranges(parent)
        rows = ["node\ti\tj\ttips\ttotal\tjoint\tgain"]
        for q, node in enumerate(self.py_nodes):
            kids = np.flatnonzero(parent == node)
            size = hi[kids] - lo[kids] + 1
            total, joint = self.py_total[q].sum(axis=2), self.py_joint[q].sum(axis=2)
            for i in range(len(kids)):
                for j in range(i + 1, len(kids)):
                    rows.append(f"{node}\t{i}\t{j}\t{size[i] + size[j]}\t{total[i, j]}\t{joint[i, j]}"
                                f"\t{2 * joint[i, j] - total[i, j]}")
        return "\n".join(rows) + "\n"

    def resolve_polytomies(self, min_gain: int = 1):
        """The greedy resolution of the scored polytomies from the tensors held here (``resolve.ResolveResult``; no
        device call).  ``initial_distance`` / ``predicted_distance`` are None unless the triplet terms were computed."""
        self._need_polytomies()
        from spectralclustersupertree_amd.resolve import resolve_from_tensors

        initial = self.total_triplet_distance if self.t_shared is not None else None
        return resolve_from_tensors(self.supertree, self.py_nodes, self.py_total, self.py_joint, self.py_skipped,
                                    initial, min_gain)

    # resampled / weighted branch triplet support (``branch_resample=...`` or ``tree_weights=...``; None otherwise),
    # kept beside the dataclass fields like ``_py``: a dict with the keys of ``_RS_KEYS``
    _rs = None

    def _rs_counter(self, x: int, rows: bool) -> np.ndarray | None:
        got = None if self._rs is None else self._rs["rs_rows" if rows else "rs_point"]
        return None if got is None else got[x]

    @property
    def rs_weights(self) -> np.ndarray | None:
        """The R x trees weight matrix that was scored, columns in the order of ``trees`` as given: row 0 the point
        estimate's weights, the others the replicates."""
        return None if self._rs is None else self._rs["rs_weights"]

    @property
    def rs_total(self) -> np.ndarray | None:
        """Per node, row 0: ``bt_total`` with every source counted ``tree_weights`` times."""
        return self._rs_counter(0, False)

    @property
    def rs_concordant(self) -> np.ndarray | None:
        return self._rs_counter(1, False)

    @property
    def rs_alt1(self) -> np.ndarray | None:
        return self._rs_counter(2, False)

    @property
    def rs_alt2(self) -> np.ndarray | None:
        return self._rs_counter(3, False)

    @property
    def rs_total_rows(self) -> np.ndarray | None:
        """R x nodes: every row of ``rs_weights`` (``resample_rows=True``; None otherwise)."""
        return self._rs_counter(0, True)

    @property
    def rs_concordant_rows(self) -> np.ndarray | None:
        return self._rs_counter(1, True)

    @property
    def rs_alt1_rows(self) -> np.ndarray | None:
        return self._rs_counter(2, True)

    @property
    def rs_alt2_rows(self) -> np.ndarray | None:
        return self._rs_counter(3, True)

    @property
    def rs_wins(self) -> dict | None:
        """``win_concordant``, ``win_alt1``, ``win_alt2``, ``win_tie`` per node: the informative replicates (rs_total
        > 0 there) by the arrangement whose count is strictly greatest, or tied.  None without replicates."""
        return None if self._rs is None else self._rs["rs_wins"]

    @property
    def branch_support(self) -> np.ndarray | None:
        """``win_concordant`` over the informative replicates per node (NaN where there is none)."""
        wins = self.rs_wins
        if wins is None:
            return None
        n = sum(wins.values())
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 0, wins["win_concordant"] / np.maximum(n, 1), np.nan)

    def annotate_branch_support(self) -> TreeNode:
        """A copy of the supertree whose quartet branches are named by their ``branch_support`` in percent (one
        decimal; no name where no replicate is informative) and whose other internal nodes carry no name, so that
        ``get_newick(with_node_names=True)`` writes it.  ``ValueError`` unless replicates were scored."""
        values = self.branch_support
        if values is None:
            msg = "no replicates were scored: score_supertree(..., branch_resample=N)"
            raise ValueError(msg)
        out = self.supertree.copy()
        mask = self.quartet_branch
        for i, node in enumerate(_preorder(out)):
            if node.is_tip():
                continue
            node.name = f"{100.0 * values[i]:.1f}" if mask[i] and not np.isnan(values[i]) else None
        return out

    def branch_table(self) -> str:
        """One TSV row per quartet branch: node (preorder index), clade_size, informative, supported, decisive,
        concordant, alt1, alt2, other, then bt_total, bt_concordant, bt_alt1, bt_alt2 when the branch triplet counts
        were computed, then win_concordant, win_alt1, win_alt2, win_tie, support when replicates were scored.
        ``ValueError`` unless the concordance was computed."""
        self._need_concordance()
        bt = self.bt_total is not None
        wins, support = self.rs_wins, self.branch_support
        nodes = _preorder(self.supertree)
        size = np.array([1 if v.is_tip() else 0 for v in nodes], dtype=np.int64)
        parent = self.supertree.to_flat()[0]
        for i in range(len(nodes) - 1, 0, -1):
            size[parent[i]] += size[i]
        other = self.other
        rows = ["node\tclade_size\tinformative\tsupported\tdecisive\tconcordant\talt1\talt2\tother"
                + ("\tbt_total\tbt_concordant\tbt_alt1\tbt_alt2" if bt else "")
                + ("\twin_concordant\twin_alt1\twin_alt2\twin_tie\tsupport" if wins else "")]
        for i in np.flatnonzero(self.quartet_branch):
            row = (f"{i}\t{size[i]}\t{self.informative[i]}\t{self.supported[i]}\t{self.decisive[i]}"
                   f"\t{self.concordant[i]}\t{self.alt1[i]}\t{self.alt2[i]}\t{other[i]}")
            if bt:
                row += f"\t{self.bt_total[i]}\t{self.bt_concordant[i]}\t{self.bt_alt1[i]}\t{self.bt_alt2[i]}"
            if wins:
                row += "".join(f"\t{wins[k][i]}" for k in _WIN_KEYS) + f"\t{support[i]:.4f}"
            rows.append(row)
        return "\n".join(rows) + "\n"

    # MRP parsimony (``parsimony=True``; None otherwise), kept beside the dataclass fields like ``_py``: a dict with the
    # four per-tree counts, ``chars`` (None, or per source tree the ``len``, ``lo``, ``hi`` arrays of its characters) and
    # ``source`` (index -> that source tree as a tree object)
    _mrp = None

    def _mrp_count(self, key: str) -> np.ndarray | None:
        return None if self._mrp is None else self._mrp[key]

    @property
    def mrp_chars(self) -> np.ndarray | None:
        """Per source tree: its characters, the nontrivial clusters (= ``n_source``)."""
        return self._mrp_count("mrp_chars")

    @property
    def mrp_length(self) -> np.ndarray | None:
        """Per source tree: the parsimony length of the supertree on its characters."""
        return self._mrp_count("mrp_length")

    @property
    def mrp_perfect(self) -> np.ndarray | None:
        """Per source tree: its characters of length 1, the clusters the supertree displays (= ``shared``)."""
        return self._mrp_count("mrp_perfect")

    @property
    def mrp_max(self) -> np.ndarray | None:
        """Per source tree: the length of its characters on a star, the most any supertree can need."""
        return self._mrp_count("mrp_max")

    def _need_parsimony(self, chars: bool = False) -> None:
        if self._mrp is None:
            msg = "parsimony scores were not computed: score_supertree(..., parsimony=True)"
            raise ValueError(msg)
        if chars and self._mrp["chars"] is None:
            msg = "per-clade lengths were not computed: score_supertree(..., parsimony=True, parsimony_chars=True)"
            raise ValueError(msg)

    @property
    def mrp_extra(self) -> np.ndarray:
        """Per source tree: the changes beyond one per character (0: the supertree displays the whole tree)."""
        self._need_parsimony()
        return self.mrp_length - self.mrp_chars

    @property
    def total_mrp_length(self) -> int:
        """The MRP supertree score: the length over every source's characters."""
        self._need_parsimony()
        return int(self.mrp_length.sum())

    @property
    def consistency_index(self) -> float:
        """Σ chars / Σ length over all sources (NaN without a character)."""
        self._need_parsimony()
        return consistency(int(self.mrp_chars.sum()), int(self.mrp_length.sum()))

    @property
    def tree_consistency_index(self) -> np.ndarray:
        """``mrp_chars / mrp_length`` per source tree (NaN where it has no character)."""
        self._need_parsimony()
        return consistency(self.mrp_chars, self.mrp_length)

    @property
    def retention_index(self) -> float:
        """(Σ max - Σ length) / (Σ max - Σ chars) over all sources (NaN where no character can take two changes)."""
        self._need_parsimony()
        return retention(int(self.mrp_chars.sum()), int(self.mrp_length.sum()), int(self.mrp_max.sum()))

    @property
    def tree_retention_index(self) -> np.ndarray:
        """The same per source tree."""
        self._need_parsimony()
        return retention(self.mrp_chars, self.mrp_length, self.mrp_max)

    def parsimony_table(self) -> str:
        """One TSV row per source tree: index, n_leaves, mrp_chars, mrp_length, mrp_perfect, mrp_max, mrp_extra,
        consistency_index, retention_index.  ``ValueError`` unless the parsimony scores were computed."""
        ci, ri = self.tree_consistency_index, self.tree_retention_index
        rows = ["index\tn_leaves\tmrp_chars\tmrp_length\tmrp_perfect\tmrp_max\tmrp_extra\tconsistency_index"
                "\tretention_index"]
        for t in range(len(ci)):
            rows.append(f"{t}\t{self.n_leaves[t]}\t{self.mrp_chars[t]}\t{self.mrp_length[t]}\t{self.mrp_perfect[t]}"
                        f"\t{self.mrp_max[t]}\t{self.mrp_extra[t]}\t{ci[t]:.4f}\t{ri[t]:.4f}")
        return "\n".join(rows) + "\n"

    def mrp_char_length(self, i: int) -> np.ndarray:
        """The length of every character of source tree ``i`` (as given), in the order of the clusters' first gaps
        in the tree's DFS order."""
        self._need_parsimony(chars=True)
        return self._mrp["chars"][int(i)]["len"]

    def mrp_char_clusters(self, i: int) -> list:
        """The clusters behind ``mrp_char_length(i)``: one list of tip names each, in the tree's DFS order."""
        self._need_parsimony(chars=True)
        got = self._mrp["chars"][int(i)]
        if len(got["len"]) == 0:
            return []
        names = self._mrp["source"](int(i)).get_tip_names()
        return [names[lo:hi + 1] for lo, hi in zip(got["lo"], got["hi"])]

    def worst_source_clades(self, n: int | None = None) -> list[dict]:
        """Every source clade with its length: one dict per character with ``tree`` (index as given), ``tips`` (its
        names), ``size``, ``length`` and ``gmax``; largest length first, then the larger gmax, then tree and character
        order.  The first ``n`` when given."""
        self._need_parsimony(chars=True)
        rows = []
        for i, got in enumerate(self._mrp["chars"]):
            if len(got["len"]) == 0:
                continue
            m = int(self.n_leaves[i])
            size = got["hi"].astype(np.int64) - got["lo"] + 1
            gmax = np.minimum(size, m - size + 1)
            rows += [(-int(got["len"][j]), -int(gmax[j]), i, j) for j in range(len(size))]
        rows.sort()
        out, clusters = [], {}
        for length, gmax, i, j in rows if n is None else rows[:n]:
            if i not in clusters:
                clusters[i] = self.mrp_char_clusters(i)
            tips = clusters[i][j]
            out.append({"tree": i, "tips": tips, "size": len(tips), "length": -length, "gmax": -gmax})
        return out

    def source_clade_table(self, n: int | None = None) -> str:
        """``worst_source_clades`` as TSV: tree, tips (comma-separated), size, length, gmax."""
        rows = ["tree\ttips\tsize\tlength\tgmax"]
        for r in self.worst_source_clades(n):
            rows.append(f"{r['tree']}\t{','.join(r['tips'])}\t{r['size']}\t{r['length']}\t{r['gmax']}")
        return "\n".join(rows) + "\n"

    def annotate_source(self, i: int) -> TreeNode:
        """A copy of source tree ``i`` whose inner nodes with a nontrivial cluster are named by that cluster's length
        on the supertree (no name elsewhere), so that ``get_newick(with_node_names=True)`` writes it."""
        self._need_parsimony(chars=True)
        out = self._mrp["source"](int(i)).copy()
        length = {frozenset(c): int(x) for c, x in zip(self.mrp_char_clusters(i), self.mrp_char_length(i))}
        for node in _preorder(out):
            if not node.is_tip():
                got = length.get(frozenset(node.get_tip_names()))
                node.name = None if got is None else str(got)
        return out

    def table(self) -> str:
        """One TSV row per source tree: index, n_leaves, n_super, n_source, shared, rf, then t_super, t_source,
        t_shared, triplet_distance when the triplet terms were computed, n_super_conflict, n_source_conflict
        when the conflicts were, n_decisive, n_concordant, n_alternative when the concordance was and n_bt_total,
        n_bt_concordant, n_bt_alternative when the branch triplet counts were and mrp_chars, mrp_length, mrp_perfect,
        mrp_max when the parsimony scores were."""
        mrp = self._mrp is not None
        trip = self.t_shared is not None
        bt = self.n_bt_total is not None
        conf = self.n_super_conflict is not None
        conc = self.n_decisive is not None
        head = "index\tn_leaves\tn_super\tn_source\tshared\trf"
        if trip:
            head += "\tt_super\tt_source\tt_shared\ttriplet_distance"
        if conf:
            head += "\tn_super_conflict\tn_source_conflict"
        if conc:
            head += "\tn_decisive\tn_concordant\tn_alternative"
        if bt:
            head += "\tn_bt_total\tn_bt_concordant\tn_bt_alternative"
        if mrp:
            head += "\tmrp_chars\tmrp_length\tmrp_perfect\tmrp_max"
        rows = [head]
        rf = self.rf
        td = self.triplet_distance if trip else None
        for t in range(len(rf)):
            row = f"{t}\t{self.n_leaves[t]}\t{self.n_super[t]}\t{self.n_source[t]}\t{self.shared[t]}\t{rf[t]}"
            if trip:
                row += f"\t{self.t_super[t]}\t{self.t_source[t]}\t{self.t_shared[t]}\t{td[t]}"
            if conf:
                row += f"\t{self.n_super_conflict[t]}\t{self.n_source_conflict[t]}"
            if conc:
                row += f"\t{self.n_decisive[t]}\t{self.n_concordant[t]}\t{self.n_alternative[t]}"
            if bt:
                row += f"\t{self.n_bt_total[t]}\t{self.n_bt_concordant[t]}\t{self.n_bt_alternative[t]}"
            if mrp:
                row += f"\t{self.mrp_chars[t]}\t{self.mrp_length[t]}\t{self.mrp_perfect[t]}\t{self.mrp_max[t]}"
            rows.append(row)
        return "\n".join(rows) + "\n"


def _preorder(tree: TreeNode) -> list[TreeNode]:
    """Nodes in the order of ``TreeNode.to_flat``."""
    out: list[TreeNode] = []
    stack = [tree]
    while stack:
        node = stack.pop()
        out.append(node)
        stack.extend(reversed(node.children))
    return out


def consistency(chars, length):
    """chars / length (a float for ints, an array for arrays); NaN where the length is 0."""
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(np.asarray(length) > 0, np.asarray(chars) / np.maximum(length, 1), np.nan)
    return float(out) if out.ndim == 0 else out


def retention(chars, length, most):
    """(most - length) / (most - chars); NaN where most = chars (no character can take a second change)."""
    room = np.asarray(most) - np.asarray(chars)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(room > 0, (np.asarray(most) - np.asarray(length)) / np.maximum(room, 1), np.nan)
    return float(out) if out.ndim == 0 else out


def _at(children: list, node: TreeNode) -> int:
    """The position of ``node`` itself among ``children``."""
    return [c is node for c in children].index(True)


def _move_clade(root: TreeNode, clade: TreeNode, goal: TreeNode, replaced: dict | None = None) -> TreeNode:
    """Prunes the subtree of ``clade`` and regrafts it on the edge above ``goal``, in place in the tree of ``root`` (a
    copy the caller owns; ``goal`` is not inside the clade), and returns the root, which the move may replace.  Nodes
    are compared by identity.  The node the clade leaves behind is suppressed when it keeps one child (``replaced``,
    when given, then maps its ``id`` to that child); when ``goal`` is that node, the clade goes above the remaining
    child.  Nothing moves when ``goal`` holds no taxon outside the clade (a unary ancestor) or the clade holds every
    taxon.  The new node holds ``[goal, clade]``."""
    # prune: the clade, the nodes it leaves empty, and the node it leaves with one child
    gone = clade
    while gone.parent is not None and len(gone.parent.children) == 1:
        if gone.parent is goal:
            return root
        gone = gone.parent
    above = gone.parent
    if above is None:
        return root
    del above.children[_at(above.children, gone)]
    clade.parent = None
    if len(above.children) == 1:
        (kid,) = above.children
        if replaced is not None:
            replaced[id(above)] = kid
        if goal is above:
            goal = kid
        kid.parent = above.parent
        if above.parent is None:
            root = kid
        else:
            sibs = above.parent.children
            sibs[_at(sibs, above)] = kid
    # regraft: a new node above the target, holding the target and the clade
    up = goal.parent
    new = TreeNode(None)
    if up is None:
        root = new
    else:
        up.children[_at(up.children, goal)] = new
        new.parent = up
    new.append(goal)
    new.append(clade)
    return root


def _best_node(row: np.ndarray, own: int) -> tuple[int, int]:
    """``(node, distance)`` of the best place in one row of distances: the smallest distance; among equals the query's
    ``own`` node, else the lowest preorder index."""
    low = int(row.min())
    return (own if row[own] == low else int(np.argmin(row))), low


def _leaf_ranges(parent: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """First and last tip (taxon id = position among the tips in preorder) below every preorder node."""
    n = len(parent)
    has_child = np.zeros(n, dtype=bool)
    has_child[parent[1:]] = True
    lo = np.full(n, n, dtype=np.int64)
    hi = np.full(n, -1, dtype=np.int64)
    tips = np.flatnonzero(~has_child)
    lo[tips] = hi[tips] = np.arange(len(tips))
    for v in range(n - 1, 0, -1):
        u = parent[v]
        lo[u] = min(lo[u], lo[v])
        hi[u] = max(hi[u], hi[v])
    return lo, hi


def quartet_branches(parent: np.ndarray) -> np.ndarray:
    """Bool mask over preorder nodes given their ``parent`` array (root -1): the nodes with exactly two children
    whose parent has exactly two children."""
    parent = np.asarray(parent, dtype=np.int64)
    kids = np.bincount(parent[1:], minlength=len(parent))
    mask = np.zeros(len(parent), dtype=bool)
    mask[1:] = (kids[1:] == 2) & (kids[parent[1:]] == 2)
    return mask


def supertree_arrays(supertree: TreeNode) -> tuple[np.ndarray, np.ndarray, list[str]]:
    """``(parent, taxon, tips)``: the supertree's preorder arrays over taxon ids = positions in ``tips``
    (its tip names in preorder).  ``ValueError`` for a nameless or repeated tip."""
    parents, names, _, _ = supertree.to_flat()
    parent = np.asarray(parents, dtype=np.int32)
    n = len(parent)
    has_child = np.zeros(n, dtype=bool)
    has_child[parent[1:]] = True
    taxon = np.full(n, -1, dtype=np.int32)
    tips: list[str] = []
    for v in np.flatnonzero(~has_child):
        name = names[v]
        if name is None or name == "":
            msg = "every tip of the supertree needs a name"
            raise ValueError(msg)
        taxon[v] = len(tips)
        tips.append(name)
    if len(set(tips)) != len(tips):
        msg = "the supertree holds a taxon more than once"
        raise ValueError(msg)
    return parent, taxon, tips


def score_supertree(supertree: TreeNode, trees, *, triplets: bool = False, conflicts: bool = False,
                    concordance: bool = False, branch_triplets: bool = False, taxon_triplets: bool = False,
                    placements=None, clade_placements=None, clade_max_tips: int = 64, polytomies=None,
                    polytomy_max_degree: int = 64, branch_resample=None, tree_weights=None,
                    resample: str = "bootstrap", resample_seed: int = 0, resample_rows: bool = False,
                    parsimony: bool = False, parsimony_chars: bool = False, device=None) -> SupertreeScore:
    """RF distance of ``supertree`` to every source tree and the support of every clade (module docstring);
    ``triplets=True`` adds the rooted triplet terms (``t_super``, ``t_source``, ``t_shared``) and
    ``conflicts=True`` the clade conflict counts (``n_super_conflict``, ``n_source_conflict``, ``conflicting``) and
    ``concordance=True`` the branch concordance counts (``n_decisive``, ``n_concordant``, ``n_alternative`` per
    tree, ``decisive``, ``concordant``, ``alt1``, ``alt2`` per node) and ``branch_triplets=True`` the per-branch
    triplet support (``n_bt_total``, ``n_bt_concordant``, ``n_bt_alternative`` per tree, ``bt_total``,
    ``bt_concordant``, ``bt_alt1``, ``bt_alt2`` per node) and ``taxon_triplets=True`` the per-taxon triplet support
    (``taxa``, ``tx_trees``, ``tx_total``, ``tx_super``, ``tx_source``, ``tx_shared`` per supertree tip), all counted
    on the same device tables as the RF terms.  ``placements``: a list of tip names, or an int N for the N least
    stable taxa (``rogue_taxa(N)``: largest ``taxon_instability`` among the taxa some source of 3 or more leaves
    holds; this implies ``taxon_triplets=True``): the placement support of those taxa (``pl_taxa``, ``pl_trees``,
    ``pl_total``, ``pl_source`` per query, ``pl_super``, ``pl_shared`` per query and supertree node).  ``ValueError``
    for an unknown or repeated name.  ``clade_placements``: a list whose items are preorder node indices or iterables
    of tip names that are exactly one node's cluster (the topmost such node), or an int N for N clades picked by
    ``select_clades`` from the per-taxon counts (this implies ``taxon_triplets=True``; ``clade_max_tips`` bounds
    their size): the clade placement support of those nodes (``cp_nodes``, ``cp_trees``, ``cp_total``, ``cp_source``
    per query, ``cp_super``, ``cp_shared`` per query and supertree node).  ``ValueError`` for the root, a node out of
    range or given twice, or names that are no node's cluster.  ``polytomies``: True for every node with three or more
    children, or a list whose items are preorder node indices or iterables of tip names that are exactly the cluster
    of such a node: what the sources say about grouping the children (``py_nodes``, ``py_degree``, ``py_trees`` per
    polytomy, ``py_total``, ``py_joint`` one k x k x k array each; ``polytomy_table``, ``polytomy_merge_gain``,
    ``resolve_polytomies``).  Polytomies of more than ``polytomy_max_degree`` (at most 64) children, or whose rows of
    the largest source do not fit a workgroup's LDS, are not scored and listed in ``py_skipped``.  ``ValueError`` for
    a node with fewer than three children, out of range or given twice.  ``branch_resample``: a replicate count N or
    an explicit N x trees matrix of non-negative integer weights, and / or ``tree_weights``: one non-negative integer
    per tree (both in the order of ``trees`` as given; integral floats are taken, anything else is a ``ValueError``:
    scoring is exact and takes integer weights): the per-branch triple counts under those weights (``rs_weights``,
    ``rs_total``, ``rs_concordant``, ``rs_alt1``, ``rs_alt2``: row 0, the point estimate under ``tree_weights``;
    ``rs_wins`` and ``branch_support`` over the replicates; ``rs_total_rows`` and so on, R x nodes, with
    ``resample_rows=True``; ``annotate_branch_support``, ``nni_candidates(by="triplets", min_support=p)``).  The
    replicates of a count are drawn by ``resample_weights`` (``resample``: ``"bootstrap"`` or ``"jackknife"``, from
    ``numpy.random.RandomState(resample_seed)``).  With ``tree_weights`` alone there is row 0 and no replicate.
    ``parsimony=True``: the MRP parsimony scores (``mrp_chars``, ``mrp_length``, ``mrp_perfect``, ``mrp_max`` per tree;
    ``mrp_extra``, ``total_mrp_length``, ``consistency_index``, ``retention_index``, ``parsimony_table``);
    ``parsimony_chars=True`` (which implies it) also the length of every source clade (``mrp_char_length``,
    ``mrp_char_clusters``, ``worst_source_clades``, ``annotate_source``).

    ``trees``: a list of tree objects (``NotCompleted`` entries dropped, as in ``construct_supertree``) or a
    ``TreeArrays`` (``load_tree_arrays``), whose tables are then built on the device.  Tree weights are accepted
    by those inputs and ignored: every count is unweighted but those of ``branch_resample`` / ``tree_weights``, which
    take the weights given here.  The supertree must hold every taxon of every source
    tree exactly once (``ValueError`` otherwise); it may hold taxa no source has.  ``device``: a
    ``backend.Device``; default the process's device (in a launched multi-rank job the caller's own: scoring is
    not spread over ranks).
    """
    t0 = time.perf_counter()
    parent, taxon, tips = supertree_arrays(supertree)
    index = {name: i for i, name in enumerate(tips)}
    placements = _check_placements(placements, index)
    clades = _check_clade_placements(clade_placements, parent, index, clade_max_tips)
    req = _Request(triplets, conflicts, concordance, branch_triplets,
                   taxon_triplets or isinstance(placements, int) or isinstance(clades, int), placements, clades,
                   clade_max_tips, tips, _check_polytomies(polytomies, parent, index, polytomy_max_degree),
                   int(polytomy_max_degree),
                   resample=None if branch_resample is None and tree_weights is None else resample_weights(
                       _n_given(trees), branch_resample, tree_weights, resample, resample_seed),
                   resample_rows=bool(resample_rows), parsimony=bool(parsimony or parsimony_chars),
                   parsimony_chars=bool(parsimony_chars))
    with _resident_tables(device, trees, tips, index) as src:
        timings = {"prepare": 0.0, "tables": src.seconds}
        res = _run_passes(src, parent, taxon, req, timings)
    timings["prepare"] = time.perf_counter() - t0 - sum(timings.values())
    return _result(supertree, src.n_leaves, res, timings, trees)


_COUNTS = tuple(f.name for f in fields(SupertreeScore) if f.name not in ("supertree", "n_leaves", "timings"))


_PY_KEYS = ("py_nodes", "py_degree", "py_trees", "py_total", "py_joint", "py_skipped")


def _source_getter(trees):
    """index -> the source tree of that index as a tree object, for either input of ``score_supertree``."""
    if isinstance(trees, TreeArrays):
        return trees.to_tree
    kept = [t for t in trees if not is_not_completed(t)]
    return kept.__getitem__


def _result(supertree, n_leaves, res: dict, timings: dict, trees=None) -> SupertreeScore:
    out = SupertreeScore(supertree=supertree, n_leaves=n_leaves, timings=timings,
                         **{k: res.get(k) for k in _COUNTS})
    if "mrp_chars" in res:
        out._mrp = {k: res[k] for k in _MRP_KEYS}
        out._mrp["chars"] = res.get("mrp_char_rows")
        out._mrp["source"] = None if trees is None else _source_getter(trees)
    if "py_nodes" in res:
        out._py = {k: res[k] for k in _PY_KEYS}
    if "rs_point" in res:
        out._rs = {k: res[k] for k in _RS_KEYS}
    return out


_RS_KEYS = ("rs_weights", "rs_point", "rs_wins", "rs_rows")
_MRP_KEYS = ("mrp_chars", "mrp_length", "mrp_perfect", "mrp_max")
_WIN_KEYS = ("win_concordant", "win_alt1", "win_alt2", "win_tie")


def _n_given(trees) -> int:
    """The trees ``score_supertree`` counts in ``trees``: what its weights have one entry for."""
    return trees.n_trees if isinstance(trees, TreeArrays) else sum(not is_not_completed(t) for t in trees)


def _integers(values, what: str) -> np.ndarray:
    """``values`` as int64 when they are non-negative integers (integral floats included)."""
    a = np.asarray(values)
    ok = a.dtype != bool and (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating))
    if not ok or not np.all(np.isfinite(a)) or np.any(a != np.floor(a)) or np.any(a < 0):
        msg = f"{what} must be non-negative integers: scoring is exact and takes integer weights"
        raise ValueError(msg)
    return a.astype(np.int64)


def resample_weights(n_trees: int, branch_resample=None, tree_weights=None, resample: str = "bootstrap",
                     seed: int = 0) -> np.ndarray | None:
    """The R x ``n_trees`` int64 weight matrix ``score_supertree`` scores for these arguments, or None when neither
    ``branch_resample`` nor ``tree_weights`` is given.  Row 0 = ``tree_weights`` (ones by default).  An explicit
    ``branch_resample`` matrix gives rows 1 .. R - 1 as they are.  A count N draws them one after the other from
    ``rs = numpy.random.RandomState(seed)``: ``"bootstrap"``: ``rs.multinomial(n_trees, numpy.full(n_trees,
    1 / n_trees)) * tree_weights`` (n_trees draws with replacement); ``"jackknife"``: ``rs.randint(0, 2, n_trees) *
    tree_weights`` (each tree kept with probability 1/2)."""
    if branch_resample is None and tree_weights is None:
        return None
    if resample not in ("bootstrap", "jackknife"):
        msg = f"resample must be 'bootstrap' or 'jackknife', not {resample!r}"
        raise ValueError(msg)
    m = int(n_trees)
    if m == 0:  # (nothing to weight: ``score_supertree`` refuses an empty list itself)
        return None
    point = np.ones(m, dtype=np.int64) if tree_weights is None else _integers(tree_weights, "tree_weights")
    if point.shape != (m,):
        msg = f"tree_weights must have one entry per source tree ({m}), not shape {point.shape}"
        raise ValueError(msg)
    if branch_resample is None:
        reps = np.zeros((0, m), dtype=np.int64)
    elif np.ndim(branch_resample) == 0:
        n = _integers(branch_resample, "branch_resample")
        rs = np.random.RandomState(seed)
        if resample == "bootstrap":
            draws = [rs.multinomial(m, np.full(m, 1.0 / m)) for _ in range(int(n))]
        else:
            draws = [rs.randint(0, 2, m) for _ in range(int(n))]
        reps = np.array(draws, dtype=np.int64).reshape(int(n), m) * point
    else:
        reps = _integers(branch_resample, "branch_resample")
        if reps.ndim != 2 or reps.shape[1] != m:
            msg = f"a branch_resample matrix must be replicates x source trees ({m}), not shape {reps.shape}"
            raise ValueError(msg)
    return np.vstack([point[None, :], reps])


def _check_placements(placements, index: dict):
    """``None``, a count or the query taxon ids of ``score_supertree``'s ``placements``."""
    if placements is None:
        return None
    if isinstance(placements, (bool, str)):
        msg = "placements must be a list of taxon names or a count"
        raise ValueError(msg)
    if isinstance(placements, (int, np.integer)):
        if placements < 0:
            msg = f"placements = {placements} is negative"
            raise ValueError(msg)
        return int(placements)
    ids = []
    for name in placements:
        if name not in index:
            msg = f"placement taxon {name!r} is not in the supertree"
            raise ValueError(msg)
        ids.append(index[name])
    if len(set(ids)) != len(ids):
        msg = "a placement taxon is given more than once"
        raise ValueError(msg)
    return np.array(ids, dtype=np.int32)


def _placement_queries(placements, res: dict, tips) -> np.ndarray:
    """The query taxon ids: as given, or the least stable taxa of the per-taxon counts in ``res``."""
    if not isinstance(placements, int):
        return placements
    view = SupertreeScore(None, None, None, None, None, None, None, taxa=list(tips), tx_trees=res["tx_trees"],
                          tx_total=res["tx_total"], tx_super=res["tx_super"], tx_source=res["tx_source"],
                          tx_shared=res["tx_shared"])
    return np.array([r["taxon"] for r in view.rogue_taxa(placements)], dtype=np.int32)


def _no_rows(prefix: str, nq: int, n_nodes: int) -> dict:
    """The ``pl_*`` / ``cp_*`` counts of ``nq`` queries that were not sent to the device: zeros."""
    out = {f"{prefix}_{k}": np.zeros(nq, dtype=np.int64) for k in ("trees", "total", "source")}
    out.update({f"{prefix}_{k}": np.zeros((nq, n_nodes), dtype=np.int64) for k in ("super", "shared")})
    return out


def _placements(dev, tabs, parent, taxon, res: dict, req) -> dict:
    queries = _placement_queries(req.placements, res, req.tips)
    out = {"pl_taxa": queries.astype(np.int64)}
    if len(queries) == 0 or tabs is None:
        out.update(_no_rows("pl", len(queries), len(parent)))
    else:
        out.update(dev.score_placements(tabs, parent, taxon, queries, batch_trees=BATCH_TREES or 0,
                                        lds_bytes=PLACEMENT_LDS_BYTES or 0))
    return out


def _check_clade_placements(clades, parent: np.ndarray, index: dict, max_tips):
    """``None``, a count or the query nodes (preorder indices) of ``score_supertree``'s ``clade_placements``."""
    if clades is None:
        return None
    if isinstance(clades, (bool, str)):
        msg = "clade_placements must be a list of nodes or name sets, or a count"
        raise ValueError(msg)
    if isinstance(clades, (int, np.integer)):
        if clades < 0 or int(max_tips) < 2:
            msg = f"clade_placements = {clades} is negative or clade_max_tips = {max_tips} is under 2"
            raise ValueError(msg)
        return int(clades)
    lo, hi = _leaf_ranges(parent.astype(np.int64))
    by_range: dict = {}
    for v in range(len(parent) - 1, -1, -1):  # (the topmost node of a range wins)
        by_range[(int(lo[v]), int(hi[v]))] = v
    nodes = []
    for item in clades:
        if isinstance(item, (int, np.integer)) and not isinstance(item, bool):
            if not 1 <= int(item) < len(parent):
                msg = f"clade node {item} is the root or not in [1, {len(parent)})"
                raise ValueError(msg)
            nodes.append(int(item))
            continue
        names = [item] if isinstance(item, str) else list(item)
        ids = set()
        for name in names:
            if name not in index:
                msg = f"clade taxon {name!r} is not in the supertree"
                raise ValueError(msg)
            ids.add(index[name])
        key = (min(ids), max(ids)) if ids else None
        if key is None or len(ids) != len(names) or key[1] - key[0] + 1 != len(ids) or key not in by_range:
            msg = f"the names {sorted(names)!r} are not exactly one node's cluster"
            raise ValueError(msg)
        if by_range[key] == 0:
            msg = "a clade to place may not be the whole supertree"
            raise ValueError(msg)
        nodes.append(by_range[key])
    if len(set(nodes)) != len(nodes):
        msg = "a clade node is given more than once"
        raise ValueError(msg)
    return np.array(nodes, dtype=np.int32)


def select_clades(n: int, parent, instability, tx_trees, max_tips: int = 64) -> np.ndarray:
    """The ``n`` clades ``clade_placements=n`` scores, as preorder node indices: the non-root nodes with 2 to
    ``max_tips`` tips, ranked by the mean ``taxon_instability`` of their tips over those with ``tx_trees`` >= 1 and a
    defined instability (a clade without one is no candidate), largest first, then the larger clade, then the lower
    preorder index; taken greedily, skipping a node nested in or containing one already taken."""
    parent = np.asarray(parent, dtype=np.int64)
    lo, hi = _leaf_ranges(parent)
    inst = np.asarray(instability, dtype=np.float64)
    ok = (np.asarray(tx_trees) >= 1) & ~np.isnan(inst)
    total = np.concatenate([[0.0], np.cumsum(np.where(ok, inst, 0.0))])
    count = np.concatenate([[0], np.cumsum(ok)])
    size = hi - lo + 1
    ranked = []
    for v in range(1, len(parent)):
        held = count[hi[v] + 1] - count[lo[v]]
        if 2 <= size[v] <= max_tips and held > 0:
            ranked.append((-(total[hi[v] + 1] - total[lo[v]]) / held, -int(size[v]), v))
    ranked.sort()
    taken: list[int] = []
    for _, _, v in ranked:
        if len(taken) == n:
            break
        if all(hi[v] < lo[u] or hi[u] < lo[v] for u in taken):
            taken.append(v)
    return np.array(taken, dtype=np.int32)


def _clade_queries(clades, parent, res: dict, max_tips) -> np.ndarray:
    if not isinstance(clades, int):
        return clades
    dist = res["tx_super"] + res["tx_source"] - 2 * res["tx_shared"]
    both = res["tx_super"] + res["tx_source"]
    with np.errstate(invalid="ignore", divide="ignore"):
        inst = np.where(both > 0, dist / np.maximum(both, 1), np.nan)
    return select_clades(clades, parent, inst, res["tx_trees"], max_tips)


def _clade_placements(dev, tabs, parent, taxon, res: dict, req) -> dict:
    queries = _clade_queries(req.clades, parent, res, req.clade_max_tips)
    out = {"cp_nodes": queries.astype(np.int64)}
    if len(queries) == 0 or tabs is None:
        out.update(_no_rows("cp", len(queries), len(parent)))
    else:
        out.update(dev.score_clade_placements(tabs, parent, taxon, queries, batch_trees=BATCH_TREES or 0,
                                              lds_bytes=CLADE_PLACEMENT_LDS_BYTES or 0))
    return out


PY_MAX_DEGREE = 64        # children of a polytomy the sweep has lanes for
PY_LDS_BYTES = 160 << 10  # all the LDS a workgroup can take


def _check_polytomies(polytomies, parent: np.ndarray, index: dict, max_degree):
    """``None``, True or the query nodes (preorder indices) of ``score_supertree``'s ``polytomies``."""
    if polytomies is None or polytomies is False:
        return None
    if not 3 <= int(max_degree) <= PY_MAX_DEGREE:
        msg = f"polytomy_max_degree = {max_degree} is not in [3, {PY_MAX_DEGREE}]"
        raise ValueError(msg)
    if polytomies is True:
        return True
    if isinstance(polytomies, (str, int, np.integer)):
        msg = "polytomies must be True or a list of nodes or name sets"
        raise ValueError(msg)
    kids = np.bincount(parent[1:], minlength=len(parent)) if len(parent) > 1 else np.zeros(len(parent), dtype=int)
    lo, hi = _leaf_ranges(parent.astype(np.int64))
    by_range: dict = {}
    for v in range(len(parent)):  # (of a chain of unary nodes the lowest can have the children)
        by_range[(int(lo[v]), int(hi[v]))] = v
    nodes = []
    for item in polytomies:
        if isinstance(item, (int, np.integer)) and not isinstance(item, bool):
            if not 0 <= int(item) < len(parent):
                msg = f"polytomy node {item} is not in [0, {len(parent)})"
                raise ValueError(msg)
            node = int(item)
        else:
            names = [item] if isinstance(item, str) else list(item)
            ids = set()
            for name in names:
                if name not in index:
                    msg = f"polytomy taxon {name!r} is not in the supertree"
                    raise ValueError(msg)
                ids.add(index[name])
            key = (min(ids), max(ids)) if ids else None
            if key is None or len(ids) != len(names) or key[1] - key[0] + 1 != len(ids) or key not in by_range:
                msg = f"the names {sorted(names)!r} are not exactly one node's cluster"
                raise ValueError(msg)
            node = by_range[key]
        if kids[node] < 3:
            msg = f"node {node} has {kids[node]} children: not a polytomy"
            raise ValueError(msg)
        nodes.append(node)
    if len(set(nodes)) != len(nodes):
        msg = "a polytomy node is given more than once"
        raise ValueError(msg)
    return np.array(nodes, dtype=np.int32)


def polytomy_queries(parent, nodes, max_degree: int, max_leaves: int, lds_bytes: int = 0):
    """``(sent, skipped)``: of the polytomies ``nodes`` (True: every node of ``parent`` with three or more children)
    those ``scs_score_polytomies`` takes, and dicts ``node``, ``degree``, ``reason`` for those over ``max_degree``
    children or whose k rows of a source of ``max_leaves`` leaves, 8 k ceil(max_leaves / 32) bytes, do not fit a
    workgroup's LDS (``lds_bytes`` > 0: that many bytes)."""
    parent = np.asarray(parent, dtype=np.int64)
    kids = np.bincount(parent[1:], minlength=len(parent)) if len(parent) > 1 else np.zeros(len(parent), dtype=int)
    if nodes is True:
        nodes = np.flatnonzero(kids >= 3)
    cap = min(int(lds_bytes), PY_LDS_BYTES) if lds_bytes and lds_bytes > 0 else PY_LDS_BYTES
    words = max((int(max_leaves) + 31) // 32, 1)
    sent, skipped = [], []
    for v in np.asarray(nodes, dtype=np.int64):
        k = int(kids[v])
        if k > max_degree:
            skipped.append({"node": int(v), "degree": k, "reason": f"more than {max_degree} children"})
        elif 8 * k * words > cap:
            skipped.append({"node": int(v), "degree": k,
                            "reason": f"{k} rows of a source of {int(max_leaves)} leaves take {8 * k * words} bytes "
                                      f"of LDS, more than {cap}"})
        else:
            sent.append(int(v))
    return np.array(sent, dtype=np.int32), skipped


def _polytomies(dev, tabs, parent, taxon, res: dict, req) -> dict:
    lds = POLYTOMY_LDS_BYTES or 0
    sent, skipped = polytomy_queries(parent, req.polytomies, req.polytomy_max_degree, req.max_leaves, lds)
    out = {"py_nodes": sent.astype(np.int64), "py_skipped": skipped}
    if len(sent) == 0 or tabs is None:
        kids = np.bincount(np.asarray(parent[1:], dtype=np.int64), minlength=len(parent))[sent]
        out.update({"py_degree": kids.astype(np.int32), "py_trees": np.zeros(len(sent), dtype=np.int64),
                    "py_total": [np.zeros((k, k, k), dtype=np.int64) for k in kids],
                    "py_joint": [np.zeros((k, k, k), dtype=np.int64) for k in kids]})
    else:
        out.update(dev.score_polytomies(tabs, parent, taxon, sent, batch_trees=BATCH_TREES or 0, lds_bytes=lds))
    return out


def _default_device():
    from spectralclustersupertree_amd.scs import default_device

    return default_device()


@dataclass
class _Sources:
    """What ``_resident_tables`` yields: the device, the source tables on it (None when no source tree has two
    leaves), the leaf count of every source tree as given, the wall seconds the tables took and, for a ``TreeArrays``
    input, the split forest the tables were made from."""

    dev: object
    tabs: object
    n_leaves: np.ndarray
    seconds: float
    forest: object = None

    def tree_index(self) -> np.ndarray | None:
        """``TreeArrays`` input: the given tree behind every tree of the tables (trees of fewer than two leaves have
        none).  None for tree objects, whose tables hold every tree in its place."""
        return None if self.forest is None else np.array(self.forest.tables()[4], dtype=np.int64)


@contextmanager
def _resident_tables(device, trees, tips: list, index: dict):
    """The source tables on the device over the taxon ids of ``index`` (name -> id; ``tips`` = the names by id), for
    either input of ``score_supertree`` and with its checks, which come before the first device call (``device``
    None: the process's device, asked for after them).  A ``TreeArrays`` forest is uploaded and restricted to all of
    its taxa in one part (``scs_forest_split``), which renumbers them to the ids of ``index`` and flattens every tree
    in HBM.  Yields a ``_Sources``; the tables are freed on the way out."""
    if isinstance(trees, TreeArrays):
        import ctypes as C

        from spectralclustersupertree_amd import _native as nv
        from spectralclustersupertree_amd.backend import DeviceForest, DeviceTables

        if trees.n_trees == 0:
            msg = "There must be at least one tree to score against."
            raise ValueError(msg)
        n_taxa = len(tips)
        # (the forest's id range is widened to the supertree's: the split's parts may not hold more taxa than it)
        universe = max(trees.n_taxa, n_taxa, 1)
        new_id = np.full(universe, -1, dtype=np.int32)
        for x in trees.present_taxa():
            name = trees.name(int(x))
            if name not in index:
                msg = f"taxon {name!r} of a source tree is not in the supertree"
                raise ValueError(msg)
            new_id[int(x)] = index[name]
        dev = device if device is not None else _default_device()
        t0 = time.perf_counter()
        n_leaves = trees.leaf_counts().astype(np.int64)
        forest = DeviceForest.upload(
            dev, universe, np.ascontiguousarray(trees.node_off, dtype=np.int64),
            np.ascontiguousarray(trees.parent, dtype=np.int32), np.ascontiguousarray(trees.taxon, dtype=np.int32),
            np.ascontiguousarray(trees.length, dtype=np.float64), np.ascontiguousarray(trees.support, dtype=np.float64),
            np.ones(trees.n_trees, dtype=np.float64), int(n_leaves.sum()))
        try:
            part_of = np.where(new_id >= 0, 0, -1).astype(np.int32)
            (child,) = forest.split(part_of, new_id, [n_taxa], 0)
        finally:
            forest.free()
        try:
            if child.n_trees == 0:  # (every tree has fewer than two leaves: nothing to count)
                yield _Sources(dev, None, n_leaves, time.perf_counter() - t0)
                return
            handle = C.c_void_p()
            nv.check(dev._lib.scs_tables_from_forest(dev._ctx, child._h, None, int(n_taxa), C.byref(handle)))
            tabs = DeviceTables(dev, handle, int(n_taxa), child.n_trees)
            try:
                yield _Sources(dev, tabs, n_leaves, time.perf_counter() - t0, child)
            finally:
                tabs.free()
        finally:
            child.free()
        return
    trees = [t for t in trees if not is_not_completed(t)]
    if len(trees) == 0:
        msg = "There must be at least one tree to score against."
        raise ValueError(msg)
    for tree in trees:
        for name in tree.get_tip_names():
            if name not in index:
                msg = f"taxon {name!r} of a source tree is not in the supertree"
                raise ValueError(msg)
    tables = flatten_trees(trees, [1.0] * len(trees), "one", taxa=tips)
    dev = device if device is not None else _default_device()
    t0 = time.perf_counter()
    tabs = dev.upload(tables)
    try:
        yield _Sources(dev, tabs, np.diff(tables.tree_off), time.perf_counter() - t0)
    finally:
        tabs.free()


@dataclass(frozen=True)
class _Request:
    """What one ``score_supertree`` call asks for, after its checks (``placements`` / ``clades``: None, a count or
    the query ids; ``tips``: the supertree's tip names by taxon id)."""

    triplets: bool
    conflicts: bool
    concordance: bool
    branch_triplets: bool
    taxon_triplets: bool
    placements: object
    clades: object
    clade_max_tips: int
    tips: list
    polytomies: object = None       # None, True or the query nodes
    polytomy_max_degree: int = 64
    max_leaves: int = 0             # of the largest source tree (set by ``_run_passes``)
    resample: object = None         # None or the R x trees weight matrix, columns in the order of the trees as given
    resample_rows: bool = False
    tree_index: object = None       # the given tree behind every tree of the tables (set by ``_run_passes``)
    parsimony: bool = False
    parsimony_chars: bool = False
    n_given: int = 0                # the source trees as given (set by ``_run_passes``)


@dataclass(frozen=True)
class _Pass:
    """One scoring pass: its key in ``timings``, whether a request wants it, the call ``(dev, tabs, parent, taxon,
    res, req) -> dict`` (``res``: what the passes before it returned) and the names of its outputs with one entry per
    source tree, per supertree node and per supertree tip.  A pass with ``queries`` picks its queries from ``res`` and
    has one row per query; it is also called without tables (``tabs`` None) and then fills its rows with zeros."""

    key: str
    wanted: object
    run: object
    per_tree: tuple = ()
    per_node: tuple = ()
    per_tip: tuple = ()
    queries: bool = False


def _on_tables(method: str):
    """The pass that is the ``Device`` method of that name and nothing else."""
    return lambda dev, tabs, parent, taxon, res, req: getattr(dev, method)(tabs, parent, taxon,
                                                                           batch_trees=BATCH_TREES or 0)


def _taxon_triplets(dev, tabs, parent, taxon, res: dict, req) -> dict:
    return dev.score_taxon_triplets(tabs, parent, taxon, batch_trees=BATCH_TREES or 0, lds_bytes=TAXON_LDS_BYTES or 0)


def _branch_resample(dev, tabs, parent, taxon, res: dict, req) -> dict:
    w, n = req.resample, len(parent)
    if tabs is None:
        out = {"rs_point": np.zeros((4, n), dtype=np.int64), "rs_wins": np.zeros((4, n), dtype=np.int32),
               "rs_rows": np.zeros((4, len(w), n), dtype=np.int64) if req.resample_rows else None}
    else:
        out = dev.score_branch_resample(tabs, parent, taxon, w if req.tree_index is None else w[:, req.tree_index],
                                        rows=req.resample_rows, batch_trees=BATCH_TREES or 0)
    out["rs_weights"] = w
    out["rs_wins"] = dict(zip(_WIN_KEYS, out["rs_wins"])) if len(w) > 1 else None
    return out


def _parsimony(dev, tabs, parent, taxon, res: dict, req) -> dict:
    """The four per-tree counts and, with ``parsimony_chars``, ``mrp_char_rows``: per source tree as given a dict of
    its characters' ``len``, ``lo``, ``hi`` (empty for a tree the tables do not hold).  The character buffers are sized
    by ``n_source`` of the first pass."""
    out = dev.score_parsimony(tabs, parent, taxon, chars=req.parsimony_chars, batch_trees=BATCH_TREES or 0,
                              pass_words=PARSIMONY_PASS_WORDS or 0,
                              n_chars=int(res["n_source"].sum()) if req.parsimony_chars else None)
    got = {k: out[k] for k in _MRP_KEYS}
    if req.parsimony_chars:
        none = {k: np.zeros(0, dtype=np.int32) for k in ("len", "lo", "hi")}
        rows = [none] * req.n_given
        off = out["char_off"]
        for j in range(len(off) - 1):
            i = j if req.tree_index is None else int(req.tree_index[j])
            rows[i] = {k: out["char_" + k][off[j]:off[j + 1]] for k in ("len", "lo", "hi")}
        got["mrp_char_rows"] = rows
    return got


# in call order (the query passes read the per-taxon counts)
_PASSES = (
    _Pass("score", lambda req: True, _on_tables("score"),
          ("n_super", "n_source", "shared"), ("informative", "supported")),
    _Pass("triplets", lambda req: req.triplets, _on_tables("score_triplets"), ("t_super", "t_source", "t_shared")),
    _Pass("conflicts", lambda req: req.conflicts, _on_tables("score_conflicts"),
          ("n_super_conflict", "n_source_conflict"), ("conflicting",)),
    _Pass("concordance", lambda req: req.concordance, _on_tables("score_concordance"),
          ("n_decisive", "n_concordant", "n_alternative"), ("decisive", "concordant", "alt1", "alt2")),
    _Pass("branch_triplets", lambda req: req.branch_triplets, _on_tables("score_branch_triplets"),
          ("n_bt_total", "n_bt_concordant", "n_bt_alternative"), ("bt_total", "bt_concordant", "bt_alt1", "bt_alt2")),
    _Pass("taxon_triplets", lambda req: req.taxon_triplets, _taxon_triplets,
          per_tip=("tx_trees", "tx_total", "tx_super", "tx_source", "tx_shared")),
    _Pass("placements", lambda req: req.placements is not None, _placements, queries=True),
    _Pass("clade_placements", lambda req: req.clades is not None, _clade_placements, queries=True),
    _Pass("polytomies", lambda req: req.polytomies is not None, _polytomies, queries=True),
    _Pass("branch_resample", lambda req: req.resample is not None, _branch_resample, queries=True),
    _Pass("parsimony", lambda req: req.parsimony, _parsimony, _MRP_KEYS),
)


def _run_passes(src: _Sources, parent, taxon, req: _Request, timings: dict) -> dict:
    """Runs the passes ``req`` wants on the tables of ``src`` and times each into ``timings``.  Counts per source tree
    go back to the places of the trees as given (``src.tree_index``); without tables every output is zeros."""
    m = len(src.n_leaves)
    tree_index = None if src.tabs is None else src.tree_index()
    req = replace(req, max_leaves=int(np.max(src.n_leaves)) if m else 0, tree_index=tree_index, n_given=m)
    res: dict = {}
    for p in _PASSES:
        if not p.wanted(req):
            continue
        t = time.perf_counter()
        if src.tabs is not None or p.queries:
            out = p.run(src.dev, src.tabs, parent, taxon, res, req)
        else:
            sized = ((p.per_tree, m), (p.per_node, len(parent)), (p.per_tip, len(req.tips)))
            out = {k: np.zeros(n, dtype=np.int64) for names, n in sized for k in names}
        timings[p.key] = time.perf_counter() - t
        if tree_index is not None:
            for k in p.per_tree:
                full = np.zeros(m, dtype=np.int64)
                full[tree_index] = out[k]
                out[k] = full
        res.update(out)
    if req.taxon_triplets or req.placements is not None:
        res["taxa"] = list(req.tips)
    if req.parsimony_chars and "mrp_char_rows" not in res:  # (no tables: no tree has a character)
        res["mrp_char_rows"] = [{k: np.zeros(0, dtype=np.int32) for k in ("len", "lo", "hi")}] * m
    return res


# ------------------------------------------------------------------------------------- the sources against one another
def _normalized(rf: np.ndarray, total: np.ndarray) -> np.ndarray:
    out = np.full(rf.shape, np.nan, dtype=np.float64)
    np.divide(rf, total, out=out, where=total > 0)
    return out


@dataclass
class SourceDistances:
    """The Robinson-Foulds terms between source trees, every pair restricted to the taxa both trees hold
    (``source_distances``).  Row i is tree ``rows[i]`` of the trees as given, column j tree j.
    With L the taxa both trees hold and C(X|L) the distinct sets cl(v) ∩ L of 2 <= size < |L| over the nodes v of X:
    ``common`` = |L|, ``clusters`` = |C(row|L)|, ``clusters_other`` = |C(column|L)|, ``shared`` = the sets in both
    (int32, rows x trees; fewer than 3 common taxa: zeros beside ``common``).

    With ``triplets=True`` also the rooted-triplet terms of every pair (int64, rows x trees, None
    otherwise): ``triplets`` / ``triplets_other`` = the triples of L that the row / column tree resolves,
    ``triplets_shared`` = those both resolve the same way."""

    common: np.ndarray
    clusters: np.ndarray
    clusters_other: np.ndarray
    shared: np.ndarray
    rows: np.ndarray
    n_leaves: np.ndarray
    timings: dict = field(default_factory=dict)
    triplets: np.ndarray | None = None
    triplets_other: np.ndarray | None = None
    triplets_shared: np.ndarray | None = None

    @property
    def rf(self) -> np.ndarray:
        """Robinson-Foulds distance of every pair on its common taxa (int64)."""
        return self.clusters.astype(np.int64) + self.clusters_other - 2 * self.shared.astype(np.int64)

    @property
    def normalized_rf(self) -> np.ndarray:
        """``rf`` / (``clusters`` + ``clusters_other``); NaN where neither restricted tree has a cluster."""
        return _normalized(self.rf, self.clusters.astype(np.int64) + self.clusters_other)

    def _need_triplets(self) -> None:
        if self.triplets is None or self.triplets_other is None or self.triplets_shared is None:
            msg = "the triplet matrices are not there: ask source_distances for triplets=True"
            raise ValueError(msg)

    @property
    def triples_total(self) -> np.ndarray:
        """C(``common``, 3): the triples of every pair's common taxa (int64)."""
        c = self.common.astype(np.int64)
        return c * (c - 1) * (c - 2) // 6

    @property
    def triplet_distance(self) -> np.ndarray:
        """The triples of every pair's common taxa that one tree resolves and the other does not resolve that way
        (int64): ``triplets`` + ``triplets_other`` - 2 ``triplets_shared``."""
        self._need_triplets()
        return self.triplets + self.triplets_other - 2 * self.triplets_shared

    @property
    def normalized_triplet_distance(self) -> np.ndarray:
        """``triplet_distance`` / (``triplets`` + ``triplets_other``); NaN where neither restricted tree resolves a
        triple."""
        return _normalized(self.triplet_distance, self.triplets + self.triplets_other)

    def _normalized_by(self, by: str) -> np.ndarray:
        if by == "rf":
            return self.normalized_rf
        if by == "triplets":
            self._need_triplets()
            return self.normalized_triplet_distance
        msg = f"by must be 'rf' or 'triplets', not {by!r}"
        raise ValueError(msg)

    def _comparable(self, min_common: int, by: str = "rf") -> np.ndarray:
        ok = (self.common >= int(min_common)) & ~np.isnan(self._normalized_by(by))
        ok[np.arange(len(self.rows)), self.rows] = False  # (a tree is not compared with itself)
        return ok

    def mean_distance(self, min_common: int = 4, by: str = "rf") -> tuple[np.ndarray, np.ndarray]:
        """``(mean, comparable)`` per row: the mean normalized RF (``by="triplets"``: the mean normalized triplet
        distance) to the other trees that share at least ``min_common`` taxa with it (and have a cluster, or a
        resolved triple, to compare; NaN when there is none) and how many those are."""
        ok = self._comparable(min_common, by)
        comparable = ok.sum(axis=1).astype(np.int64)
        total = np.where(ok, np.nan_to_num(self._normalized_by(by)), 0.0).sum(axis=1)
        return _normalized(total, comparable), comparable

    def outlier_sources(self, n: int | None = None, min_common: int = 4, by: str = "rf") -> list[dict]:
        """The rows by ``mean_distance`` (of ``by``), the worst first (ties by tree; trees with nothing to compare
        left out): dicts ``tree``, ``mean_distance``, ``comparable``; the first ``n`` of them."""
        mean, comparable = self.mean_distance(min_common, by)
        order = sorted((i for i in range(len(self.rows)) if comparable[i] > 0),
                       key=lambda i: (-mean[i], int(self.rows[i])))
        out = [{"tree": int(self.rows[i]), "mean_distance": float(mean[i]), "comparable": int(comparable[i])}
               for i in order]
        return out if n is None else out[: max(int(n), 0)]

    def table(self, min_common: int = 3) -> str:
        """TSV, one row per unordered pair of trees a < b with at least ``min_common`` (>= 3) common taxa that a row
        of the matrices holds: tree_a, tree_b, common, clusters_a, clusters_b, shared, rf, normalized_rf -- and, when
        the triplet matrices are there, triplets_a, triplets_b, triplets_shared, triplet_distance,
        normalized_triplet_distance."""
        floor = max(int(min_common), 3)
        trip = self.triplets is not None
        lines = ["tree_a\ttree_b\tcommon\tclusters_a\tclusters_b\tshared\trf\tnormalized_rf"]
        if trip:
            self._need_triplets()
            lines[0] += "\ttriplets_a\ttriplets_b\ttriplets_shared\ttriplet_distance\tnormalized_triplet_distance"
        first = {}
        for i, r in enumerate(self.rows.tolist()):
            first.setdefault(r, i)
        found = {}
        for r, i in first.items():
            for j in np.flatnonzero(self.common[i] >= floor).tolist():
                if j == r or (j < r and j in first):
                    continue  # (itself, or the pair is listed from the other tree's row)
                mine, other = int(self.clusters[i, j]), int(self.clusters_other[i, j])
                a, b, ca, cb = (r, j, mine, other) if r < j else (j, r, other, mine)
                found[(a, b)] = (int(self.common[i, j]), ca, cb, int(self.shared[i, j]))
                if trip:
                    mine, other = int(self.triplets[i, j]), int(self.triplets_other[i, j])
                    found[(a, b)] += (*((mine, other) if r < j else (other, mine)), int(self.triplets_shared[i, j]))
        for (a, b), (c, ca, cb, sh, *more) in sorted(found.items()):
            rf = ca + cb - 2 * sh
            nrf = f"{rf / (ca + cb):.4f}" if ca + cb else "nan"
            lines.append(f"{a}\t{b}\t{c}\t{ca}\t{cb}\t{sh}\t{rf}\t{nrf}")
            if trip:
                ta, tb, ts = more
                td = ta + tb - 2 * ts
                ntd = f"{td / (ta + tb):.4f}" if ta + tb else "nan"
                lines[-1] += f"\t{ta}\t{tb}\t{ts}\t{td}\t{ntd}"
        return "\n".join(lines) + "\n"


def _source_names(trees) -> list[str]:
    """The taxon names of the sources, each once, in order of first appearance."""
    if isinstance(trees, TreeArrays):
        return [trees.name(int(x)) for x in trees.present_taxa()]
    seen: dict = {}
    for tree in trees:
        if not is_not_completed(tree):
            for name in tree.get_tip_names():
                seen.setdefault(name, None)
    return list(seen)


def source_distances(trees, rows=None, device=None, triplets: bool = False) -> SourceDistances:
    """The Robinson-Foulds terms between every two source trees, each pair restricted to the taxa both trees hold:
    which sources disagree with the rest, which pairs overlap too little to say anything (``SourceDistances``).

    ``trees``: a list of tree objects (``NotCompleted`` entries dropped) or a ``TreeArrays``, as for
    ``score_supertree``; the taxon ids are the union of their names.  ``rows``: the trees (indices into ``trees`` as
    given) whose rows are wanted, in any order; None: all of them.  Trees of fewer than two leaves of a ``TreeArrays``
    have no tables: their rows and columns are zeros.  Every count comes from ``scs_score_source_pairs``; with
    ``triplets`` the rooted-triplet terms of every pair come from ``scs_score_source_pair_triplets`` as well (the
    graded measure: one misplaced taxon breaks every cluster on its path, but only the triples it is in)."""
    t0 = time.perf_counter()
    names = _source_names(trees)
    index = {name: i for i, name in enumerate(names)}
    keys = ("common", "clusters", "clusters_other", "shared")
    tkeys = ("triplets", "triplets_other", "triplets_shared") if triplets else ()
    with _resident_tables(device, trees, names, index) as src:
        m = len(src.n_leaves)
        given = np.arange(m, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
        if given.ndim != 1 or (given.size and (given.min() < 0 or given.max() >= m)):
            msg = f"rows must be indices of the {m} source trees"
            raise ValueError(msg)
        out = {k: np.zeros((len(given), m), dtype=np.int32) for k in keys}
        out.update({k: np.zeros((len(given), m), dtype=np.int64) for k in tkeys})
        timings = {"prepare": 0.0, "tables": src.seconds, "pairs": 0.0}
        if triplets:
            timings["triplets"] = 0.0
        if src.tabs is not None and len(given):
            tree_index = src.tree_index()
            t1 = time.perf_counter()
            if tree_index is None:
                ask = None if rows is None else given.astype(np.int32)
                res = src.dev.score_source_pairs(src.tabs, ask)
                out.update({k: res[k] for k in keys})
                timings["pairs"] = time.perf_counter() - t1
                if triplets:
                    res = src.dev.score_source_pair_triplets(src.tabs, ask, outputs=tkeys)
                    out.update({k: res[k] for k in tkeys})
            else:
                at = np.full(m, -1, dtype=np.int64)
                at[tree_index] = np.arange(len(tree_index))
                have = np.flatnonzero(at[given] >= 0)
                ask = at[given[have]].astype(np.int32)
                everything = len(ask) == len(tree_index) and np.array_equal(ask, np.arange(len(tree_index)))
                if len(ask):
                    res = src.dev.score_source_pairs(src.tabs, None if everything else ask)
                    for k in keys:
                        out[k][np.ix_(have, tree_index)] = res[k]
                timings["pairs"] = time.perf_counter() - t1
                if triplets and len(ask):
                    res = src.dev.score_source_pair_triplets(src.tabs, None if everything else ask, outputs=tkeys)
                    for k in tkeys:
                        out[k][np.ix_(have, tree_index)] = res[k]
            if triplets:
                timings["triplets"] = time.perf_counter() - t1 - timings["pairs"]
    timings["prepare"] = time.perf_counter() - t0 - sum(timings.values())
    return SourceDistances(rows=given, n_leaves=np.asarray(src.n_leaves, dtype=np.int64), timings=timings, **out)


# ------------------------------------------------------------------------------------- the triple coverage of the sources
@dataclass
class SourceCoverage:
    """Which taxa the sources ever show together (``source_coverage``).  M[x] is the set of
    trees that hold taxon x; cov(a, b, c) = |M[a] ∩ M[b] ∩ M[c]|; a triple of three distinct taxa is *covered* when
    cov >= k, with k = ``min_trees`` >= 1.  Row i is taxon ``rows[i]``; taxon ids index ``taxa``.

    ``occurs[x]`` = |M[x]| for all taxa; ``taxon_covered[i]`` the covered triples that contain the row's taxon,
    ``taxon_triples`` = C(n - 1, 2) the triples that do, ``taxon_coverage`` their ratio (NaN for n < 3).  With every
    taxon a row (``rows`` None): ``triples_total`` = C(n, 3), ``triples_covered``, ``coverage`` and ``decisive`` (every
    triple covered: the taxon sets alone leave no rooted tree undetermined); None otherwise.  With ``pairs``:
    ``pair_trees[i][b]`` = |M[a] ∩ M[b]| (the diagonal is ``occurs[a]``) and ``pair_covered[i][b]`` =
    #{c ∉ {a, b} : cov(a, b, c) >= k} (the diagonal is 0), int32, rows x taxa; None otherwise."""

    taxa: list
    rows: np.ndarray
    min_trees: int
    occurs: np.ndarray
    taxon_covered: np.ndarray
    taxon_triples: int
    triples_total: int | None = None
    triples_covered: int | None = None
    pair_trees: np.ndarray | None = None
    pair_covered: np.ndarray | None = None
    timings: dict = field(default_factory=dict)

    @property
    def taxon_coverage(self) -> np.ndarray:
        """``taxon_covered`` / ``taxon_triples``; NaN with fewer than three taxa."""
        return _normalized(self.taxon_covered.astype(np.float64),
                           np.full(len(self.rows), float(self.taxon_triples)))

    @property
    def coverage(self) -> float | None:
        """``triples_covered`` / ``triples_total`` (NaN with fewer than three taxa); None unless every taxon is a row."""
        if self.triples_total is None:
            return None
        return self.triples_covered / self.triples_total if self.triples_total else float("nan")

    @property
    def decisive(self) -> bool | None:
        """Every triple is covered (None unless every taxon is a row)."""
        return None if self.triples_total is None else self.triples_covered == self.triples_total

    def least_covered_taxa(self, n: int | None = None, min_occurs: int = 1) -> list[dict]:
        """The rows by ``taxon_covered``, the worst first (ties by taxon id; each taxon once; taxa in fewer than
        ``min_occurs`` trees left out): dicts ``taxon``, ``name``, ``occurs``, ``covered``, ``coverage``; the first
        ``n`` of them."""
        first: dict = {}
        for i, r in enumerate(self.rows.tolist()):
            first.setdefault(r, i)
        ratio = self.taxon_coverage
        order = sorted((i for r, i in first.items() if self.occurs[r] >= int(min_occurs)),
                       key=lambda i: (int(self.taxon_covered[i]), int(self.rows[i])))
        out = [{"taxon": int(self.rows[i]), "name": self.taxa[int(self.rows[i])],
                "occurs": int(self.occurs[self.rows[i]]), "covered": int(self.taxon_covered[i]),
                "coverage": float(ratio[i])} for i in order]
        return out if n is None else out[: max(int(n), 0)]

    def never_together(self) -> list[tuple]:
        """The pairs (a, b) of taxon ids, a < b, that no tree holds together (``pair_trees`` == 0), each once, among
        the pairs a row of the matrices holds.  It needs ``pairs=True``."""
        if self.pair_trees is None:
            msg = "never_together needs the pair matrices: source_coverage(..., pairs=True)"
            raise ValueError(msg)
        i, b = np.nonzero(self.pair_trees == 0)
        a = self.rows[i]
        keep = a != b
        pairs = np.unique(np.stack([np.minimum(a, b)[keep], np.maximum(a, b)[keep]], axis=1), axis=0)
        return [(int(x), int(y)) for x, y in pairs.tolist()]

    def table(self) -> str:
        """TSV, one row per row taxon: taxon, occurs, covered, triples, coverage."""
        lines = ["taxon\toccurs\tcovered\ttriples\tcoverage"]
        ratio = self.taxon_coverage
        for i, r in enumerate(self.rows.tolist()):
            cov = "nan" if np.isnan(ratio[i]) else f"{ratio[i]:.4f}"
            lines.append(f"{self.taxa[r]}\t{self.occurs[r]}\t{self.taxon_covered[i]}\t{self.taxon_triples}\t{cov}")
        return "\n".join(lines) + "\n"


def _one_leaf_occurrences(trees, index: dict, n: int) -> np.ndarray:
    """Per taxon id of ``index`` the one-leaf trees of a ``TreeArrays`` that hold it: such trees have no tables."""
    extra = np.zeros(n, dtype=np.int32)
    if isinstance(trees, TreeArrays):
        counts = trees.leaf_counts()
        taxon, node_off = np.asarray(trees.taxon), np.asarray(trees.node_off)
        for t in np.flatnonzero(counts == 1).tolist():
            ids = taxon[node_off[t]:node_off[t + 1]]
            extra[index[trees.name(int(ids[ids >= 0][0]))]] += 1
    return extra


def source_coverage(trees, min_trees: int = 1, rows=None, pairs: bool = False, device=None) -> SourceCoverage:
    """The triple coverage of the sources: do they overlap enough to determine a tree at all (``SourceCoverage``)?
    A rooted triple that no source tree holds whole can only be resolved by inference through other taxa; the share
    of covered triples is the partial decisiveness of the taxon sampling.

    ``trees``: a list of tree objects (``NotCompleted`` entries dropped) or a ``TreeArrays``, as for
    ``source_distances``; the taxon ids number the union of their names (a list: in order of first appearance; a
    ``TreeArrays``: in the order of its own ids) and are listed in ``taxa``.  A triple counts
    as covered when at least ``min_trees`` trees hold all three taxa.  ``rows``: the taxa (names or ids) whose rows are
    wanted, in any order; None: all of them, which also gives the totals.  ``pairs``: the two rows x taxa matrices as
    well.  Every count is exact and comes from ``scs_score_coverage``, whose cost is
    O(rows x taxa^2 x ceil(trees / 32)); one-leaf trees of a ``TreeArrays`` have no tables and are added to ``occurs``
    (and the diagonal of ``pair_trees``) here, so both inputs give the same numbers."""
    t0 = time.perf_counter()
    if int(min_trees) < 1:
        msg = f"min_trees = {min_trees} is less than 1"
        raise ValueError(msg)
    names = _source_names(trees)
    index = {name: i for i, name in enumerate(names)}
    n = len(names)
    if rows is None:
        given = np.arange(n, dtype=np.int64)
    else:
        rows = list(rows)
        bad = [r for r in rows if (isinstance(r, str) and r not in index)
               or (not isinstance(r, str) and not 0 <= int(r) < n)]
        if bad:
            msg = f"rows must be names or ids of the {n} taxa of the sources, not {bad[0]!r}"
            raise ValueError(msg)
        given = np.array([index[r] if isinstance(r, str) else int(r) for r in rows], dtype=np.int64)
    with _resident_tables(device, trees, names, index) as src:
        timings = {"prepare": 0.0, "tables": src.seconds, "coverage": 0.0}
        out = {"occurs": np.zeros(n, dtype=np.int32), "taxon_covered": np.zeros(len(given), dtype=np.int64),
               "pair_trees": np.zeros((len(given), n), dtype=np.int32) if pairs else None,
               "pair_covered": np.zeros((len(given), n), dtype=np.int32) if pairs else None}
        if src.tabs is not None:
            t1 = time.perf_counter()
            out = src.dev.score_coverage(src.tabs, None if rows is None else given.astype(np.int32),
                                         min_trees=int(min_trees), pairs=pairs)
            timings["coverage"] = time.perf_counter() - t1
    extra = _one_leaf_occurrences(trees, index, n)
    if extra.any():
        out["occurs"] = out["occurs"] + extra
        if pairs:
            out["pair_trees"][np.arange(len(given)), given] += extra[given]
    total = covered = None
    if rows is None:
        total, covered = n * (n - 1) * (n - 2) // 6, int(out["taxon_covered"].sum()) // 3
    timings["prepare"] = time.perf_counter() - t0 - sum(timings.values())
    return SourceCoverage(taxa=names, rows=given, min_trees=int(min_trees), occurs=out["occurs"],
                          taxon_covered=out["taxon_covered"], taxon_triples=(n - 1) * (n - 2) // 2 if n >= 3 else 0,
                          triples_total=total, triples_covered=covered, pair_trees=out["pair_trees"],
                          pair_covered=out["pair_covered"], timings=timings)


# ------------------------------------------------------------------------- the internode distances of the sources
@dataclass
class InternodeDistances:
    """The internode distances of the sources, summed per pair of taxa (``source_internode_distances``; DESIGN.md
    section 41).  For a tree T, T* is the tree of its distinct clusters (unary nodes merged away, a polytomy one
    node); d_T(a, b) is the number of edges between the leaves a and b in T*, taken in T itself and not in a
    restriction (ASTRID's convention): a cherry gives 2, in ((a,b),c) d(a,c) = 3, every pair of a star gives 2.  A
    tree of weight w counts like w copies of it.  Row i is taxon ``rows[i]``; taxon ids index ``taxa``.

    ``pair_weight[i][b]`` = Σ w_t over the trees that hold both taxa, ``dist_sum[i][b]`` = Σ w_t d_t(a, b),
    ``sq_sum[i][b]`` = Σ w_t d_t(a, b)² (int64, rows x taxa, diagonal 0; None without ``matrices``, ``sq_sum`` also
    without ``squares``); ``taxon_weight``, ``taxon_sum``, ``taxon_sq`` (None without ``squares``) their row sums and
    ``taxon_partners[i]`` = #{b : pair_weight > 0}.  Every count is exact."""

    taxa: list
    rows: np.ndarray
    taxon_weight: np.ndarray
    taxon_sum: np.ndarray
    taxon_partners: np.ndarray
    taxon_sq: np.ndarray | None = None
    pair_weight: np.ndarray | None = None
    dist_sum: np.ndarray | None = None
    sq_sum: np.ndarray | None = None
    all_rows: bool = False
    timings: dict = field(default_factory=dict)

    def _need_matrices(self, what: str) -> None:
        if self.pair_weight is None:
            msg = f"{what} needs the matrices: source_internode_distances(..., matrices=True)"
            raise ValueError(msg)

    @property
    def mean(self) -> np.ndarray:
        """``dist_sum`` / ``pair_weight`` (float64): NaN where no tree holds both taxa, 0 on the diagonal."""
        self._need_matrices("mean")
        out = _normalized(self.dist_sum.astype(np.float64), self.pair_weight.astype(np.float64))
        out[np.arange(len(self.rows)), self.rows] = 0.0
        return out

    @property
    def variance(self) -> np.ndarray:
        """The weighted variance of d over the trees of a pair, ``sq_sum`` / w - mean² (NaN where w = 0, diagonal
        0).  It needs ``squares=True``."""
        self._need_matrices("variance")
        if self.sq_sum is None:
            msg = "variance needs the squares: source_internode_distances(..., squares=True)"
            raise ValueError(msg)
        w = self.pair_weight.astype(np.float64)
        mean = _normalized(self.dist_sum.astype(np.float64), w)
        # (w Σwd² >= (Σwd)² by Cauchy-Schwarz: what falls below 0 is rounding)
        out = np.maximum(_normalized(self.sq_sum.astype(np.float64), w) - mean * mean, 0.0)
        out[w == 0] = np.nan
        out[np.arange(len(self.rows)), self.rows] = 0.0
        return out

    @property
    def taxon_mean(self) -> np.ndarray:
        """``taxon_sum`` / ``taxon_weight``: the mean distance from the row's taxon to its partners (NaN with none)."""
        return _normalized(self.taxon_sum.astype(np.float64), self.taxon_weight.astype(np.float64))

    @property
    def missing_pairs(self) -> int | None:
        """The pairs of taxa that no tree holds together (None unless every taxon is a row)."""
        if not self.all_rows:
            return None
        n = len(self.taxa)
        return n * (n - 1) // 2 - int(self.taxon_partners.astype(np.int64).sum()) // 2

    @property
    def complete(self) -> bool | None:
        """Every pair of taxa is in some tree: ``mean`` has no NaN (None unless every taxon is a row)."""
        return None if not self.all_rows else self.missing_pairs == 0

    def nearest(self, taxon, n: int | None = None) -> list[dict]:
        """The partners of ``taxon`` (a name or an id; it must be a row) by mean distance, the nearest first (ties
        by taxon id): dicts ``taxon``, ``name``, ``mean``, ``weight``; the first ``n`` of them."""
        self._need_matrices("nearest")
        x = self.taxa.index(taxon) if isinstance(taxon, str) else int(taxon)
        at = np.flatnonzero(self.rows == x)
        if len(at) == 0:
            msg = f"taxon {taxon!r} is not a row of these distances"
            raise ValueError(msg)
        i = int(at[0])
        w, d = self.pair_weight[i], self.dist_sum[i]
        order = sorted(np.flatnonzero(w > 0).tolist(), key=lambda b: (int(d[b]) / int(w[b]), b))
        out = [{"taxon": b, "name": self.taxa[b], "mean": int(d[b]) / int(w[b]), "weight": int(w[b])} for b in order]
        return out if n is None else out[: max(int(n), 0)]

    def table(self) -> str:
        """TSV, one row per row taxon: taxon, partners, weight, sum, mean."""
        lines = ["taxon\tpartners\tweight\tsum\tmean"]
        mean = self.taxon_mean
        for i, r in enumerate(self.rows.tolist()):
            m = "nan" if np.isnan(mean[i]) else f"{mean[i]:.4f}"
            lines.append(f"{self.taxa[r]}\t{self.taxon_partners[i]}\t{self.taxon_weight[i]}\t{self.taxon_sum[i]}\t{m}")
        return "\n".join(lines) + "\n"

    def to_phylip(self, path, missing: float | None = None) -> None:
        """Write ``mean`` as a square PHYLIP distance matrix (every taxon must be a row, in order).  A pair that no
        tree holds is written as ``missing``; without a fill value it is a ``ValueError``."""
        self._need_matrices("to_phylip")
        if not self.all_rows:
            msg = "to_phylip needs every taxon as a row: source_internode_distances(..., rows=None)"
            raise ValueError(msg)
        mean = self.mean
        gaps = np.isnan(mean)
        if gaps.any():
            if missing is None:
                a, b = (int(v[0]) for v in np.nonzero(gaps))
                msg = (f"{int(gaps.sum()) // 2} pairs of taxa are in no tree together (the first: {self.taxa[a]!r}, "
                       f"{self.taxa[b]!r}): give a fill value, to_phylip(path, missing=...)")
                raise ValueError(msg)
            mean = np.where(gaps, float(missing), mean)
        lines = [str(len(self.taxa))]
        lines += [" ".join([str(name)] + [f"{v:.6f}" for v in row]) for name, row in zip(self.taxa, mean)]
        with open(path, "w") as out:
            out.write("\n".join(lines) + "\n")


def source_internode_distances(trees, rows=None, tree_weights=None, squares: bool = False, matrices: bool = True,
                               device=None) -> InternodeDistances:
    """The internode distances of the sources, summed per pair of taxa (``InternodeDistances``): for every pair, how
    many trees hold both taxa, and the sum and the mean over those trees of the number of edges between the two. This
    is the average internode distance matrix of ASTRID / NJst and of average-consensus supertrees, and the input of
    FastME or any NJ program for a second opinion on a spectral supertree; the mean and the variance per pair show
    which taxa the sources place consistently and which pairs they never relate at all.

    d_T(a, b) is counted in T*, the tree of T's distinct clusters: nodes with one child are merged away, a polytomy
    is one node; a cherry gives 2, in ((a,b),c) d(a,c) = 3, every pair of a star gives 2.  It is taken in T itself, not
    in T restricted to some taxon set (ASTRID's convention).

    ``trees``: a list of tree objects (``NotCompleted`` entries dropped) or a ``TreeArrays``, as for
    ``source_coverage``; its one-leaf trees have no pairs and change nothing.  ``rows``: the taxa (names or ids) whose
    rows are wanted, in any order; None: all of them.  ``tree_weights``: non-negative integers, one per tree as given
    (integral floats are accepted); a tree of weight w counts exactly like w copies, weight 0 as absent.  ``squares``:
    the sums of squares as well (``variance``).  ``matrices`` False: only the per-taxon sums, and nothing of rows x
    taxa is allocated anywhere.  Every count is exact and comes from ``scs_score_internode``; sums past 2^63 - 1 are
    refused with a ``ValueError`` before anything is summed.

    ``source_internode_distances([supertree])`` gives a supertree's own matrix, for a residual against the sources'
    mean on the host."""
    t0 = time.perf_counter()
    names = _source_names(trees)
    index = {name: i for i, name in enumerate(names)}
    n = len(names)
    if rows is None:
        given = np.arange(n, dtype=np.int64)
    else:
        rows = list(rows)
        bad = [r for r in rows if (isinstance(r, str) and r not in index)
               or (not isinstance(r, str) and not 0 <= int(r) < n)]
        if bad:
            msg = f"rows must be names or ids of the {n} taxa of the sources, not {bad[0]!r}"
            raise ValueError(msg)
        given = np.array([index[r] if isinstance(r, str) else int(r) for r in rows], dtype=np.int64)
    weights = None
    if tree_weights is not None:
        weights = _integers(tree_weights, "tree_weights")
        m_given = trees.n_trees if isinstance(trees, TreeArrays) else len(trees)
        if weights.shape != (m_given,):
            msg = f"tree_weights must have one entry per source tree ({m_given}), not shape {weights.shape}"
            raise ValueError(msg)
        if not isinstance(trees, TreeArrays):
            weights = weights[[i for i, t in enumerate(trees) if not is_not_completed(t)]]
    keys = [k for k in ("pair_weight", "dist_sum", "sq_sum", "taxon_weight", "taxon_sum", "taxon_sq", "taxon_partners")
            if (matrices or k.startswith("taxon")) and (squares or k not in ("sq_sum", "taxon_sq"))]
    with _resident_tables(device, trees, names, index) as src:
        timings = {"prepare": 0.0, "tables": src.seconds, "internode": 0.0}
        out = {k: np.zeros(len(given) if k.startswith("taxon") else (len(given), n),
                           dtype=np.int32 if k == "taxon_partners" else np.int64) for k in keys}
        if src.tabs is not None:
            tree_index = src.tree_index()
            if weights is not None and tree_index is not None:
                weights = weights[tree_index]
            t1 = time.perf_counter()
            out = src.dev.score_internode(src.tabs, None if rows is None else given.astype(np.int32),
                                          tree_weights=weights, matrices=matrices, squares=squares)
            timings["internode"] = time.perf_counter() - t1
    timings["prepare"] = time.perf_counter() - t0 - sum(timings.values())
    return InternodeDistances(taxa=names, rows=given, all_rows=rows is None, timings=timings,
                              **{k: out.get(k) for k in ("pair_weight", "dist_sum", "sq_sum", "taxon_weight",
                                                         "taxon_sum", "taxon_sq", "taxon_partners")})
