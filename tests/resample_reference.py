"""Host reference of the resampled and weighted branch triplet support of ``score_supertree(..., branch_resample=...,
tree_weights=...)`` (helper module, not collected).

``per_tree`` runs ``branch_triplet_reference.node_sum`` on every source tree alone: C[T][x][u] = what T adds to counter
x (total, concordant, alt1, alt2) of node u.  The rows of a weight matrix W (R x trees) are ``W @ C`` in Python ints,
so nothing can overflow; ``wins`` decides every replicate r >= 1 by the rule of DESIGN.md section 26 in plain Python:
informative when the total is positive, then counted once -- for the arrangement whose count is strictly greatest, or
as a tie.  ``draws`` states the replicate weights of a count N independently of the package.
"""

from __future__ import annotations

import numpy as np
from branch_triplet_reference import PER_NODE, node_sum
from clade_placement_reference import _restricted
from conflict_reference import contract
from polytomy_reference import _with_unary
from score_reference import random_tree

from spectralclustersupertree_amd.tree import TreeNode

WIN_KEYS = ("win_concordant", "win_alt1", "win_alt2", "win_tie")


def per_tree(supertree: TreeNode, trees: list[TreeNode]) -> np.ndarray:
    """C as an object array [trees][4][nodes] of Python ints."""
    n_nodes = len(supertree.to_flat()[0])
    out = np.zeros((len(trees), 4, n_nodes), dtype=object)
    for t, tree in enumerate(trees):
        alone = node_sum(supertree, [tree])
        for x, key in enumerate(PER_NODE):
            out[t, x, :] = [int(v) for v in alone[key]]
    return out


def rows(weights, counts: np.ndarray) -> np.ndarray:
    """[4][R][nodes] object array: row r of counter x = Σ_T weights[r][T] counts[T][x]."""
    w = np.array([[int(v) for v in row] for row in np.asarray(weights)], dtype=object).reshape(len(weights), -1)
    m, _, n_nodes = counts.shape
    out = np.zeros((4, len(w), n_nodes), dtype=object)
    for x in range(4):
        out[x] = w @ counts[:, x, :] if m else 0
    return out


def wins(all_rows: np.ndarray) -> np.ndarray:
    """[4][nodes] int64: win_concordant, win_alt1, win_alt2, win_tie over the rows r >= 1."""
    _, n_rep, n_nodes = all_rows.shape
    out = np.zeros((4, n_nodes), dtype=np.int64)
    for u in range(n_nodes):
        for r in range(1, n_rep):
            total, con, alt1, alt2 = (all_rows[x][r][u] for x in range(4))
            if total <= 0:
                continue
            if con > alt1 and con > alt2:
                out[0][u] += 1
            elif alt1 > con and alt1 > alt2:
                out[1][u] += 1
            elif alt2 > con and alt2 > alt1:
                out[2][u] += 1
            else:
                out[3][u] += 1
    return out


def reference(supertree: TreeNode, trees: list[TreeNode], weights) -> dict:
    """``rs_point`` [4][nodes], ``rs_rows`` [4][R][nodes] (object arrays of Python ints) and ``rs_wins`` [4][nodes]."""
    all_rows = rows(weights, per_tree(supertree, trees))
    return {"rs_point": all_rows[:, 0, :], "rs_rows": all_rows, "rs_wins": wins(all_rows)}


def draws(n_trees: int, n: int, tree_weights=None, kind: str = "bootstrap", seed: int = 0) -> np.ndarray:
    """The (1 + n) x trees matrix of a replicate count ``n``: row 0 the tree weights (ones by default), then per
    replicate, from one ``RandomState(seed)``, a multinomial draw of ``n_trees`` trees with equal probabilities
    (bootstrap) or a fair coin per tree (jackknife), times the tree weights."""
    point = [1] * n_trees if tree_weights is None else [int(v) for v in tree_weights]
    rs = np.random.RandomState(seed)
    out = [point]
    for _ in range(n):
        if kind == "bootstrap":
            count = rs.multinomial(n_trees, np.full(n_trees, 1.0 / n_trees))
        else:
            count = rs.randint(0, 2, n_trees)
        out.append([int(c) * w for c, w in zip(count, point)])
    return np.array(out, dtype=np.int64).reshape(1 + n, n_trees)


def repeated(trees: list[TreeNode], weights_row) -> list[TreeNode]:
    """Every tree ``weights_row[t]`` times: what integer weights mean."""
    return [tree.copy() for tree, w in zip(trees, weights_row) for _ in range(int(w))]


# ------------------------------------------------------------------ cases
def resample_case(rs: np.random.RandomState):
    """``(supertree, sources)``: 8 to 30 taxa; 3 to 8 sources that are restrictions of a binary model tree with some
    edges collapsed and some unary nodes; a supertree -- the model or an unrelated binary tree -- with a few edges
    collapsed (so that quartet branches remain beside polytomies) and some unary nodes."""
    n = int(rs.randint(8, 31))
    names = [f"t{i}" for i in range(n)]
    model = random_tree(rs, names, binary=True)
    trees = []
    for _ in range(int(rs.randint(3, 9))):
        keep = set(rs.choice(names, size=int(rs.randint(4, n + 1)), replace=False).tolist())
        trees.append(_with_unary(contract(_restricted(model, keep), rs, 0.2), rs, 0.15))
    base = model if rs.rand() < 0.6 else random_tree(rs, names, binary=True)
    sup = _with_unary(contract(base, rs, float(rs.uniform(0.0, 0.25))), rs, 0.05)
    return sup, trees


def resample_cases(n: int = 40, seed: int = 26) -> list:
    """The case set the CPU and the GPU tests share."""
    rs = np.random.RandomState(seed)
    return [resample_case(rs) for _ in range(n)]


def case_weights(rs: np.random.RandomState, n_trees: int, n_rep: int) -> np.ndarray:
    """A weight matrix of small integers: row 0 positive, zeros among the others, and a last row of zeros when there
    is room for it."""
    w = rs.randint(0, 4, size=(n_rep, n_trees)).astype(np.int64)
    w[0] = rs.randint(1, 4, size=n_trees)
    if n_rep > 2:
        w[n_rep - 1] = 0
    return w
