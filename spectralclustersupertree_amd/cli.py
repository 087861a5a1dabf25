"""``scs`` command line front-end with the reference's options
(reference: src/sc_supertree/cli.py:8-39): default weighting ``branch`` (the library call
defaults to ``one``), no tree weights, no seed.  The source trees are read straight into flat
arrays by the C Newick loader -- no tree object is built for the input."""

from __future__ import annotations

from pathlib import Path

import click

from spectralclustersupertree_amd import __version__


@click.command(no_args_is_help=True)
@click.version_option(__version__)
@click.option("-i", "--in-file", required=True, help="Line-separated Newick file with the source trees (parsed straight into flat arrays).")
@click.option("-o", "--out-file", required=True, help="Where the supertree is written (Newick).")
@click.option(
    "-p",
    "--pcg-weighting",
    help="How an edge of the proper cluster graph is weighted by the LCA of its two taxa.",
    default="branch",
    type=click.Choice(["one", "depth", "branch", "bootstrap"], case_sensitive=False),
)
@click.option(
    "--disable-contraction",
    help="Keep always-together taxa as separate vertices (slower, same result up to ties).",
    default=False,
    is_flag=True,
)
@click.option("--scores-out", default=None,
              help="Also score the supertree against the sources: a TSV with one row per source tree "
                   "(index, n_leaves, n_super, n_source, shared, rf).")
@click.option("--support-out", default=None,
              help="Also write the supertree with each clade's support (supported / informative sources) as its "
                   "node name (Newick).")
@click.option("--triplets", default=False, is_flag=True,
              help="Add the rooted triplet terms to --scores-out (t_super, t_source, t_shared, triplet_distance).")
@click.option("--conflicts", default=False, is_flag=True,
              help="Add the clade conflict counts to --scores-out (n_super_conflict, n_source_conflict).")
@click.option("--conflict-out", default=None,
              help="Also write the supertree with each clade's supported/conflicting/informative source counts as "
                   "its node name (Newick).")
@click.option("--concordance", default=False, is_flag=True,
              help="Add the branch concordance counts to --scores-out (n_decisive, n_concordant, n_alternative).")
@click.option("--concordance-out", default=None,
              help="Also write the supertree with each quartet branch's concordant/alt1/alt2/decisive source counts "
                   "as its node name (Newick).")
@click.option("--branches-out", default=None,
              help="Also write a TSV with one row per quartet branch (node, clade_size, informative, supported, "
                   "decisive, concordant, alt1, alt2, other).")
@click.option("--branch-triplets", default=False, is_flag=True,
              help="Add the per-branch triplet support to --scores-out (n_bt_total, n_bt_concordant, "
                   "n_bt_alternative) and to --branches-out (bt_total, bt_concordant, bt_alt1, bt_alt2).")
@click.option("--branch-triplets-out", default=None,
              help="Also write the supertree with each quartet branch's concordant/alt1/alt2/total triple counts as "
                   "its node name (Newick).")
@click.option("--branch-resample", default=0, type=click.IntRange(min=0), metavar="N",
              help="Resample the source trees N times and count, per quartet branch, the replicates in which the "
                   "branch's concordant triples outnumber both alternatives: adds win_concordant, win_alt1, win_alt2, "
                   "win_tie and support to --branches-out; needs --branches-out or --branch-support-out.")
@click.option("--resample-seed", default=0, type=int, show_default=True,
              help="The seed of the --branch-resample draws.")
@click.option("--jackknife", default=False, is_flag=True,
              help="--branch-resample keeps each source tree with probability 1/2 instead of drawing as many trees as "
                   "there are with replacement (bootstrap).")
@click.option("--branch-support-out", default=None,
              help="Also write the supertree with each quartet branch's --branch-resample support in percent as its "
                   "node name (Newick).")
@click.option("--taxon-triplets", default=False, is_flag=True,
              help="Names the per-taxon triplet support that --taxa-out counts and writes; it switches nothing on by "
                   "itself and needs --taxa-out.")
@click.option("--taxa-out", default=None,
              help="Also write a TSV with one row per supertree tip (taxon, name, tx_trees, tx_total, tx_super, "
                   "tx_source, tx_shared, triplet_distance): the rooted triples that hold the taxon, over its sources.")
@click.option("--placements-out", default=None,
              help="Also write a TSV with one row per placed taxon (taxon, name, trees, node, distance, best_node, "
                   "best_distance, improvement): where on the supertree the least stable taxa would fit their sources "
                   "best, by rooted triplet distance.")
@click.option("--place-taxa", default=10, type=click.IntRange(min=1), show_default=True,
              help="How many of the least stable taxa --placements-out places.")
@click.option("--clade-placements-out", default=None,
              help="Also write a TSV with one row per placed clade (node, tips, trees, distance, best_node, "
                   "best_distance, improvement): where on the supertree the least stable small clades would fit "
                   "their sources best as a whole, by rooted triplet distance.")
@click.option("--place-clades", default=10, type=click.IntRange(min=1), show_default=True,
              help="How many clades --clade-placements-out places.")
@click.option("--clade-max-tips", default=64, type=click.IntRange(min=2), show_default=True,
              help="The largest clade --clade-placements-out considers.")
@click.option("--refined-out", default=None,
              help="Also refine the supertree by prune-and-regraft moves that lower its rooted triplet distance to "
                   "the source trees (refine_supertree) and write the refined tree here; -o and every other output "
                   "keep describing the constructed tree.")
@click.option("--refine-rounds", default=50, type=click.IntRange(min=0), show_default=True,
              help="The most rounds --refined-out runs.")
@click.option("--refine-log", default=None,
              help="With --refined-out: a TSV with one row per move (round, kind, node, target, tips, gain, "
                   "distance_after).")
@click.option("--polytomies-out", default=None,
              help="Also write a TSV with one row per polytomy of the supertree and pair of its children (node, i, j, "
                   "tips, total, joint, gain): what the sources' rooted triples say about grouping the two.")
@click.option("--resolved-out", default=None,
              help="Also resolve the supertree's polytomies by greedy pairwise merges that lower its rooted triplet "
                   "distance to the source trees (resolve_polytomies) and write the resolved tree here; -o and every "
                   "other output keep describing the constructed tree.")
@click.option("--resolve-min-gain", default=1, type=int, show_default=True,
              help="The least gain in triplet distance a merge of --resolved-out must have.")
@click.option("--resolve-polytomies", "resolve_first", default=False, is_flag=True,
              help="With --refined-out: resolve the polytomies before the first round (refine_supertree(resolve=True)).")
@click.option("--parsimony", default=False, is_flag=True,
              help="Add the MRP parsimony scores to --scores-out (mrp_chars, mrp_length, mrp_perfect, mrp_max): the "
                   "length of the supertree on the matrix representation of every source tree.")
@click.option("--source-clades-out", default=None,
              help="Also write a TSV with one row per clade of every source tree (tree, tips, size, length, gmax): its "
                   "parsimony length on the supertree, the worst-fitting clades first.")
@click.option("--source-distances-out", default=None,
              help="Also write a TSV with one row per pair of source trees that share 3 taxa or more (tree_a, tree_b, "
                   "common, clusters_a, clusters_b, shared, rf, normalized_rf): the Robinson-Foulds terms between the "
                   "two trees restricted to the taxa both hold.")
@click.option("--source-triplets", is_flag=True,
              help="With --source-distances-out: also the rooted-triplet terms of every pair (triplets_a, triplets_b, "
                   "triplets_shared, triplet_distance, normalized_triplet_distance), the graded measure beside RF.")
@click.option("--min-common", default=3, type=click.IntRange(min=3), show_default=True,
              help="The fewest shared taxa of a pair --source-distances-out lists (3: every pair that has a cluster to "
                   "compare; the library's mean_distance and outlier_sources start at 4, where two trees can differ).")
@click.option("--coverage-out", default=None,
              help="Also write a TSV with one row per taxon (taxon, occurs, covered, triples, coverage): of the rooted "
                   "triples that hold the taxon, how many some source tree holds whole -- whether the sources overlap "
                   "enough to determine a tree at all.")
@click.option("--coverage-min-trees", default=1, type=click.IntRange(min=1), show_default=True, metavar="K",
              help="The source trees that must hold a triple for --coverage-out to count it as covered.")
@click.option("--internode-out", default=None,
              help="Also write the sources' average internode distance matrix as a square PHYLIP file: per pair of "
                   "taxa the mean, over the source trees that hold both, of the number of edges between them (the "
                   "input of ASTRID / NJst, FastME or any NJ program).")
@click.option("--internode-missing", default=None, type=float, metavar="X",
              help="The value --internode-out writes for a pair of taxa that no source tree holds together; without "
                   "it such a pair is an error.")
@click.option("--internode-taxa-out", default=None,
              help="Also write a TSV with one row per taxon (taxon, partners, weight, sum, mean): how many taxa the "
                   "sources relate it to, and its mean internode distance to them.")
def scs(in_file: str, out_file: str, pcg_weighting: str, *, disable_contraction: bool,
        scores_out: str | None = None, support_out: str | None = None, triplets: bool = False,
        conflicts: bool = False, conflict_out: str | None = None, concordance: bool = False,
        concordance_out: str | None = None, branches_out: str | None = None, branch_triplets: bool = False,
        branch_triplets_out: str | None = None, taxon_triplets: bool = False,
        taxa_out: str | None = None, placements_out: str | None = None, place_taxa: int = 10,
        clade_placements_out: str | None = None, place_clades: int = 10, clade_max_tips: int = 64,
        refined_out: str | None = None, refine_rounds: int = 50, refine_log: str | None = None,
        polytomies_out: str | None = None, resolved_out: str | None = None, resolve_min_gain: int = 1,
        resolve_first: bool = False, branch_resample: int = 0, resample_seed: int = 0, jackknife: bool = False,
        branch_support_out: str | None = None, parsimony: bool = False,
        source_clades_out: str | None = None, source_distances_out: str | None = None,
        source_triplets: bool = False, min_common: int = 3, coverage_out: str | None = None,
        coverage_min_trees: int = 1, internode_out: str | None = None, internode_missing: float | None = None,
        internode_taxa_out: str | None = None) -> None:
    """Spectral Cluster Supertree of the source trees in IN_FILE, on the MI355X core."""
    if internode_missing is not None and not internode_out:
        msg = "--internode-missing needs --internode-out"
        raise click.UsageError(msg)
    if branch_resample and not (branches_out or branch_support_out):
        msg = "--branch-resample needs --branches-out or --branch-support-out"
        raise click.UsageError(msg)
    if (branch_support_out or jackknife) and not branch_resample:
        msg = "--branch-support-out and --jackknife need --branch-resample N"
        raise click.UsageError(msg)
    if resolve_first and not refined_out:
        msg = "--resolve-polytomies needs --refined-out"
        raise click.UsageError(msg)
    if refine_log and not refined_out:
        msg = "--refine-log needs --refined-out"
        raise click.UsageError(msg)
    if source_triplets and not source_distances_out:
        msg = "--source-triplets needs --source-distances-out"
        raise click.UsageError(msg)
    if triplets and not scores_out:
        msg = "--triplets needs --scores-out"
        raise click.UsageError(msg)
    if conflicts and not scores_out:
        msg = "--conflicts needs --scores-out"
        raise click.UsageError(msg)
    if concordance and not scores_out:
        msg = "--concordance needs --scores-out"
        raise click.UsageError(msg)
    if branch_triplets and not (scores_out or branches_out):
        msg = "--branch-triplets needs --scores-out or --branches-out"
        raise click.UsageError(msg)
    if parsimony and not scores_out:
        msg = "--parsimony needs --scores-out"
        raise click.UsageError(msg)
    if taxon_triplets and not taxa_out:
        msg = "--taxon-triplets needs --taxa-out"
        raise click.UsageError(msg)
    from spectralclustersupertree_amd import construct_supertree
    from spectralclustersupertree_amd.load import load_tree_arrays

    sources = load_tree_arrays(in_file)
    supertree = construct_supertree(
        sources,
        pcg_weighting=pcg_weighting.lower(),
        contract_edges=not disable_contraction,
    )
    from spectralclustersupertree_amd.scs import default_team

    team = default_team()
    if team is None or team.rank == 0:  # a launched job: every rank holds the tree, one writes it
        supertree.write(out_file)
        if (scores_out or support_out or conflict_out or concordance_out or branches_out or branch_triplets_out
                or taxa_out or placements_out or clade_placements_out or polytomies_out or branch_support_out
                or source_clades_out):
            from spectralclustersupertree_amd.score import score_supertree

            result = score_supertree(supertree, load_tree_arrays(in_file), triplets=triplets,
                                     conflicts=conflicts or conflict_out is not None,
                                     concordance=concordance or concordance_out is not None
                                     or branches_out is not None,
                                     branch_triplets=branch_triplets or branch_triplets_out is not None,
                                     taxon_triplets=taxa_out is not None,
                                     placements=place_taxa if placements_out else None,
                                     clade_placements=place_clades if clade_placements_out else None,
                                     clade_max_tips=clade_max_tips, polytomies=True if polytomies_out else None,
                                     branch_resample=branch_resample or None, resample_seed=resample_seed,
                                     resample="jackknife" if jackknife else "bootstrap",
                                     parsimony=parsimony or source_clades_out is not None,
                                     parsimony_chars=source_clades_out is not None)
            resampled = result._rs  # (a non-field attribute: the copies made below do not carry it)
            mrp = result._mrp       # (likewise)
            if source_clades_out:
                Path(source_clades_out).write_text(result.source_clade_table())
            if branch_support_out:
                Path(branch_support_out).write_text(
                    result.annotate_branch_support().get_newick(with_node_names=True) + "\n")
            if polytomies_out:
                Path(polytomies_out).write_text(result.polytomy_table())
            if clade_placements_out:
                Path(clade_placements_out).write_text(result.clade_placement_table())
            if placements_out:
                Path(placements_out).write_text(result.placement_table())
            if taxa_out:
                Path(taxa_out).write_text(result.taxon_table())
            if branch_triplets_out:
                Path(branch_triplets_out).write_text(
                    result.annotate_branch_triplets().get_newick(with_node_names=True) + "\n")
            if not branch_triplets:
                result = _without_branch_triplets(result)  # (the tables keep their columns of before)
            if scores_out:
                shown = result if conflicts else _without_conflicts(result)
                shown = shown if concordance else _without_concordance(shown)
                shown._mrp = mrp if parsimony else None  # (--source-clades-out alone adds no column)
                Path(scores_out).write_text(shown.table())
            if support_out:
                Path(support_out).write_text(result.annotate().get_newick(with_node_names=True) + "\n")
            if conflict_out:
                Path(conflict_out).write_text(result.annotate_counts().get_newick(with_node_names=True) + "\n")
            if concordance_out:
                Path(concordance_out).write_text(
                    result.annotate_concordance().get_newick(with_node_names=True) + "\n")
            if branches_out:
                result._rs = resampled
                Path(branches_out).write_text(result.branch_table())
        if source_distances_out:
            from spectralclustersupertree_amd.score import source_distances

            distances = source_distances(sources, triplets=source_triplets)
            Path(source_distances_out).write_text(distances.table(min_common))
        if coverage_out:
            from spectralclustersupertree_amd.score import source_coverage

            Path(coverage_out).write_text(source_coverage(sources, min_trees=coverage_min_trees).table())
        if internode_out or internode_taxa_out:
            from spectralclustersupertree_amd.score import source_internode_distances

            internode = source_internode_distances(sources, matrices=internode_out is not None)
            if internode_taxa_out:
                Path(internode_taxa_out).write_text(internode.table())
            if internode_out:
                try:
                    internode.to_phylip(internode_out, missing=internode_missing)
                except ValueError as err:
                    raise click.ClickException(str(err)) from err
        if resolved_out:
            from spectralclustersupertree_amd.resolve import resolve_polytomies

            resolve_polytomies(supertree, load_tree_arrays(in_file),
                               min_gain=resolve_min_gain).supertree.write(resolved_out)
        if refined_out:
            from spectralclustersupertree_amd.refine import refine_supertree

            refined = refine_supertree(supertree, load_tree_arrays(in_file), max_rounds=refine_rounds,
                                       resolve=resolve_first)
            refined.supertree.write(refined_out)
            if refine_log:
                Path(refine_log).write_text(refined.table())


def _without_branch_triplets(result):
    """``result`` whose tables leave the branch triplet columns out (--branch-triplets-out without
    --branch-triplets)."""
    import dataclasses

    return dataclasses.replace(result, n_bt_total=None, n_bt_concordant=None, n_bt_alternative=None, bt_total=None,
                               bt_concordant=None, bt_alt1=None, bt_alt2=None)


def _without_concordance(result):
    """``result`` whose table leaves the concordance columns out (--concordance-out or --branches-out without
    --concordance)."""
    import dataclasses

    return dataclasses.replace(result, n_decisive=None, n_concordant=None, n_alternative=None)


def _without_conflicts(result):
    """``result`` whose table leaves the conflict columns out (--conflict-out without --conflicts)."""
    import dataclasses

    return dataclasses.replace(result, n_super_conflict=None, n_source_conflict=None, conflicting=None)


if __name__ == "__main__":
    scs()
