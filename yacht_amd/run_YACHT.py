"""`yacht run` driver: sample .sig.zip + training config -> presence/absence tables.

Same arguments, checks, coverage-list handling and result layout as the reference's
src/yacht/run_YACHT.py (:24-254): `results/result_all.txt` (tab-separated, every user coverage,
unfiltered) and one table per coverage named `min_coverage{c}` (only organisms with
in_sample_est unless --show_all), plus `raw_result` with --keep_raw.  The tables go to
`results/result.xlsx` (yacht_amd.xlsx: no openpyxl needed) and to `results/sheets/<name>.tsv`.
Kept on purpose: the reference fills the column "num_exclusive_kmers_in_sample_sketch" with the
sample's MEAN ABUNDANCE (run_YACHT.py:159) — downstream tools read it that way.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys
import zipfile
from pathlib import Path

import pandas as pd

from . import _lib
from . import hypothesis_recovery_src as hr
from . import phases
from . import utils
from .utils import logger

RAW_RENAMES = {
    "acceptance_threshold_with_coverage": "acceptance_threshold_wo_coverage",
    "actual_confidence_with_coverage": "actual_confidence_wo_coverage",
    "alt_confidence_mut_rate_with_coverage": "alt_confidence_mut_rate_wo_coverage",
}


# (flag, keyword arguments of add_argument): the reference's argument set (run_YACHT.py:24-72)
ARGUMENTS = (
    ("--json", dict(type=str, required=True, help="Config json written by `yacht train`.")),
    ("--sample_file", dict(required=True, nargs="+",
                           help="Metagenomic sample in .sig.zip format.  Two or more files run as one cohort against the database "
                                "built once: results/<stem>/ per sample plus results/cohort_samples.tsv and "
                                "results/cohort_presence.tsv; the per-sample intermediate files (multisearch CSV, list files) "
                                "are not written then.")),
    ("--significance", dict(type=float, default=0.99, help="Minimum probability of individual true negative.")),
    ("--num_threads", dict(type=int, default=16, help="Host threads for file handling.")),
    ("--keep_raw", dict(action="store_true", help="Keep raw results in output file.")),
    ("--show_all", dict(action="store_true", help="Show all organisms (no matter if present) in output file.")),
    ("--min_coverage_list", dict(nargs="+", type=float, default=[1, 0.5, 0.1, 0.05, 0.01],
                                 help="Fractions of a genome's unique k-mers assumed covered by the sample, each in [0, 1].")),
    ("--outdir", dict(type=str, default=os.getcwd(), help="Where the 'results' folder is created.")),
    ("--abundance", dict(action="store_true",
                         help="Also estimate how much of each organism the sample holds: the depth (sum, mean, median of the "
                              "sample's per-hash abundances) over the k-mers exclusive to each genome, as extra columns of "
                              "every table and as results/abundance_profile.tsv.  Needs a sample sketched with abundances.")),
    ("--residual", dict(action="store_true",
                        help="Also report what of the sample the organisms called present explain: results/sample_explained.tsv "
                             "(per min_coverage: sample hashes and abundance in the database, explained by the call set, and "
                             "left over) and results/residual.sig.zip, the sample restricted to the hashes the call set of "
                             "--residual_coverage does not explain, ready for another `yacht run`.")),
    ("--residual_coverage", dict(type=float, default=None,
                                 help="The --min_coverage_list value whose call set results/residual.sig.zip is taken for "
                                      "(with --residual; default: the smallest value of the list).")),
    ("--gather", dict(action="store_true",
                      help="Also rank the organisms called present by the sample hashes each adds, a minimum set cover as "
                           "`sourmash gather` makes it: results/gather_profile.tsv (per min_coverage and rank: the organism, the "
                           "sample hashes it holds, those no higher-ranked organism took, and their abundance).  One sample file; "
                           "a cohort with --gather_top: results/<stem>/gather_profile.tsv per sample and results/cohort_gather.tsv.")),
    ("--gather_min_hits", dict(type=int, default=1,
                               help="Stop the ranking when the best remaining organism adds fewer sample hashes than this (with --gather).")),
    ("--gather_coverage", dict(type=float, nargs="+", default=None,
                               help="The --min_coverage_list values the ranking is made for (with --gather; default: all of them).")),
    ("--gather_top", dict(type=int, default=None,
                          help="Rank at most this many organisms per sample and coverage (with --gather; default: no bound).  "
                               "A cohort needs it, at most %d: its samples are ranked a block at a time on the device." % _lib.YH_GATHER_BATCH_MAX_ROWS)),
    ("--lineages", dict(type=str, default=None,
                        help="A lineage table of the reference organisms, the CSV sourmash's tax and lca commands take "
                             "(ident,superkingdom,phylum,class,order,family,genus,species[,strain]; an ident is an organism's name "
                             "or its first word).  Every sample hash is then classified by the lowest common ancestor of the "
                             "organisms that hold it: results/lca_summary.tsv, per taxon the sample hashes and abundance that "
                             "resolve exactly there and anywhere under it, and how many of its organisms were called present.  "
                             "One sample file; a cohort with --lineages_rank: results/<stem>/lca_summary.tsv per sample and "
                             "results/cohort_lca.tsv.")),
    ("--lineages_rank", dict(type=str, default=None,
                             help="The rank a cohort's lineage table is cut at (with --lineages): one of %s.  A cohort needs it: "
                                  "results/cohort_lca.tsv then holds, per sample, the hashes outside the database, those that resolve "
                                  "above the rank, and one row per taxon at the rank.  Ignored with one sample file."
                                  % ", ".join(("superkingdom", "phylum", "class", "order", "family", "genus", "species", "strain")))),
    ("--compare", dict(action="store_true",
                       help="Also compare the cohort's samples with one another (two or more sample files): "
                            "results/cohort_compare.tsv, one row per pair with the shared hashes, Jaccard, containment, "
                            "Bray-Curtis and cosine, and results/cohort_compare_<metric>.csv matrices as `sourmash compare --csv` "
                            "writes them; with --residual also results/cohort_compare_residual.tsv, the same table over the hashes "
                            "the call set of --residual_coverage does not explain.  `yacht compare` does the same without a database.")),
    ("--matrix", dict(action="store_true",
                      help="Also write the cohort's organism x sample tables (two or more sample files): "
                           "results/cohort_prevalence.tsv, per min_coverage and organism the samples it is present in, and "
                           "results/cohort_matrix_presence.tsv and results/cohort_matrix_num_matches.tsv, one row per organism "
                           "and one column per sample at --matrix_coverage; with --abundance also "
                           "results/cohort_matrix_relative_abundance.tsv.")),
    ("--matrix_coverage", dict(type=float, default=None,
                               help="The --min_coverage_list value whose wide tables are written (with --matrix; default: the "
                                    "smallest value of the list).")),
    ("--matrix_min_samples", dict(type=int, default=None,
                                  help="Keep an organism in the wide tables only if it is present in at least this many samples "
                                       "at --matrix_coverage (with --matrix; default: 1).")),
)

# messages the reference raises with (callers and its tests match on them)
MSG_NO_CONFIG = "Config file {0} does not exist. Please run make_training_data_from_sketches.py first."
MSG_BAD_COVERAGE = ("One of values in the min_coverage_list you provided {0} is not between 0 and 1. "
                    "Please check your input.")
MSG_NO_MANIFEST = ("The manifest file {0} does not exist. Please check if you are using the correct json file as input.")
MSG_ZIP_WITHOUT_MANIFEST = ("The input file {0} appears to be missing a manifest associated with it. "
                            "Try running: sourmash sig merge {0} -o <new signature with the manifest present>. "
                            "And then run YACHT using the output of that command.")
MSG_NOT_ONE_SKETCH = ("Expected exactly one signature with ksize {1} in {0}, found {2}. "
                      "Likely you will need to do something like: sourmash sig merge {0} -o <new signature with just one sketch in it>.")
MSG_SCALE_MISMATCH = "Sample scale factor does not equal genome scale factor. Please check your input."


def add_arguments(parser: argparse.ArgumentParser) -> None:
    for flag, kw in ARGUMENTS:
        parser.add_argument(flag, **kw)


def coverage_plan(min_coverage_list):
    """De-duplicated, descending coverages with 1.0 forced in front; has_raw tells whether the user
    asked for 1.0 (run_YACHT.py:175-181)."""
    covs = sorted(set(min_coverage_list), reverse=True)
    has_raw = 1.0 in covs
    if not has_raw:
        covs = [1.0] + covs
    return covs, has_raw


def write_tables(tables, results_folder: str) -> None:
    """`results/result.xlsx` -- one sheet per table, the reference's sheet names (run_YACHT.py:231-254) -- written by
    yacht_amd.xlsx (zipfile + XML: no openpyxl needed to WRITE; `pd.read_excel` reads it where openpyxl exists,
    yacht_amd.xlsx.read_xlsx anywhere), and the same tables as `results/sheets/<name>.tsv`."""
    from . import xlsx

    sheets = os.path.join(results_folder, "sheets")
    os.makedirs(sheets, exist_ok=True)
    for name, df in tables:
        df.to_csv(os.path.join(sheets, f"{name}.tsv"), sep="\t", index=False)
    xlsx.write_xlsx(os.path.join(results_folder, "result.xlsx"), tables)


def add_sample_columns(manifest: pd.DataFrame, mean_abundance, n_hashes: int, scaled: int) -> None:
    """The sample's columns of the result tables (run_YACHT.py:159-162 of the reference; the mean abundance goes into
    "num_exclusive_kmers_in_sample_sketch" on purpose, see the module docstring)."""
    manifest["num_exclusive_kmers_in_sample_sketch"] = mean_abundance
    manifest["num_total_kmers_in_sample_sketch"] = utils.get_num_kmers(mean_abundance, n_hashes, scaled, scale=False)
    manifest["sample_scale_factor"] = scaled
    manifest["min_coverage"] = 1.0


def trim_results(results):
    """The columns a result table keeps, under the names the reference writes (run_YACHT.py:215-220)."""
    return [r[[c for c in r.columns if c not in ("md5sum", "sample_scale_factor")]]
            .rename(columns={"genome_scale_factor": "scale_factor"}) for r in results]


def write_sample_results(results, covs, has_raw: bool, results_folder: str, keep_raw: bool, show_all: bool) -> None:
    """result_all.txt, result.xlsx and sheets/*.tsv of one sample from its trimmed tables (one per coverage of `covs`)."""
    user_results = results if has_raw else results[1:]
    user_covs = covs if has_raw else covs[1:]
    pd.concat(user_results, ignore_index=True).to_csv(os.path.join(results_folder, "result_all.txt"), sep="\t", index=False)
    tables = []
    if keep_raw:
        tables.append(("raw_result", results[0].rename(columns=RAW_RENAMES)))
    for cov, df in zip(user_covs, user_results):
        tables.append((f"min_coverage{cov}", df if show_all else df[df["in_sample_est"] == True]))  # noqa: E712
    write_tables(tables, results_folder)


def decompress_legacy_db(genome_dir: str, num_threads: int) -> None:
    """Databases trained by old versions list *.sig.gz: decompress them once (run_YACHT.py:184-189)."""
    listed = glob.glob(f"{genome_dir}/training_sig_files.*")
    if listed:
        df = pd.read_csv(listed[0], sep="\t", header=None)
        if len(df) and "sig.gz" in df[0].values[0]:
            pd.DataFrame([x.replace("sig.gz", "sig") for x in df[0]]).to_csv(listed[0], header=False, index=False)
            utils.decompress_all_sig_files(glob.glob(f"{genome_dir}/signatures/*.sig.gz"), num_threads)


def main(args) -> None:
    files = [args.sample_file] if isinstance(args.sample_file, str) else list(args.sample_file)
    want_residual = bool(getattr(args, "residual", False))
    if getattr(args, "compare", False) and len(files) < 2:  # (before anything is written or any device work)
        from . import compare

        raise ValueError(compare.MSG_COMPARE_NEEDS_COHORT.format(len(files)))
    if getattr(args, "matrix", False) or any(getattr(args, k, None) is not None for k in ("matrix_coverage", "matrix_min_samples")):
        from . import matrix

        matrix.matrix_options(args, len(files))  # (ValueError before anything is written or any device work)
    if want_residual or getattr(args, "residual_coverage", None) is not None:
        from . import residual

        residual_cov = residual.residual_coverage(args)  # (ValueError before anything is written or any device work)
    gather_plan = None
    if getattr(args, "gather", False) or getattr(args, "gather_coverage", None) is not None or getattr(args, "gather_top", None) is not None:
        from . import gather

        gather_plan = gather.gather_options(args, len(files))  # (ValueError before anything is written or any device work)
        gather_cap = gather.gather_top(args, len(files))
    lineages = None
    if getattr(args, "lineages", None) is not None or getattr(args, "lineages_rank", None) is not None:
        from . import taxonomy

        lineages = taxonomy.lineages_option(args, len(files))  # (ValueError before anything is written or any device work)
    if len(files) > 1:
        from . import cohort

        return cohort.main(args, files)
    json_file_path = str(Path(args.json).absolute())
    sample_file = str(Path(files[0]).absolute())
    outdir = str(Path(args.outdir).absolute())
    results_folder = os.path.join(outdir, "results")
    os.makedirs(results_folder, exist_ok=True)

    utils.check_file_existence(json_file_path, MSG_NO_CONFIG.format(json_file_path))
    with open(json_file_path) as f:
        config = json.load(f)
    manifest_file_path, genome_dir = config["manifest_file_path"], config["intermediate_files_dir"]
    scale, ksize, ani_thresh = config["scale"], config["ksize"], config["ani_thresh"]

    if not os.access(outdir, os.W_OK):
        print(f"Cannot write to the location: {outdir}.\n")
        print("Please check that you have the permission to write to this location. Exiting..\n")
        sys.exit(1)
    for x in args.min_coverage_list:
        if not (0 <= x <= 1):
            raise ValueError(MSG_BAD_COVERAGE.format(x))
    utils.check_file_existence(manifest_file_path, MSG_NO_MANIFEST.format(manifest_file_path))

    logger.info("Loading the manifest file generated from the training data.")
    with phases.phase("load_manifest"):
        manifest = pd.read_csv(manifest_file_path, sep="\t", header=0)
    with zipfile.ZipFile(sample_file, "r") as z:
        if "SOURMASH-MANIFEST.csv" not in z.namelist():
            raise FileNotFoundError(MSG_ZIP_WITHOUT_MANIFEST.format(sample_file))
    with phases.phase("load_sample"):
        try:
            sample_sig = utils.load_signature_with_ksize(sample_file, ksize)
        except ValueError:
            raise ValueError(MSG_NOT_ONE_SKETCH.format(sample_file, ksize, len(sample_file)))
        # (the reference parses the file a second time here, run_YACHT.py:150-152 -> utils.py:89-110; same tuple)
        info = (sample_file, sample_sig.name, sample_sig.md5sum(), sample_sig.minhash.mean_abundance,
                len(sample_sig.minhash), sample_sig.minhash.scaled)
    add_sample_columns(manifest, info[3], info[4], info[5])
    if scale != info[5]:
        raise ValueError(MSG_SCALE_MISMATCH)
    want_abundance = bool(getattr(args, "abundance", False))
    sample_abund = None
    if want_abundance:
        from . import abundance

        with phases.phase("load_abundances"):
            sample_abund = abundance.sample_abundances(sample_sig, sample_file)

    covs, has_raw = coverage_plan(args.min_coverage_list)

    decompress_legacy_db(genome_dir, args.num_threads)

    logger.info("Computing hypothesis recovery.")
    with phases.phase("hypothesis_recovery"):
        results = hr.hypothesis_recovery(manifest, (sample_file, sample_sig), genome_dir, covs, scale, ksize,
                                         args.significance, ani_thresh, args.num_threads,
                                         **({"abundances": sample_abund} if want_abundance else {}))
    if want_residual:  # one more call on the still-resident database: the call sets are this run's presence calls
        with phases.phase("explain"):
            user_covs = covs if has_raw else covs[1:]
            call_sets = residual.call_sets_of(manifest["organism_name"], results if has_raw else results[1:])
            explained = residual.explain_call_sets(hr._LAST_RUN["db"], hr._LAST_RUN["mins"],
                                                   residual.sample_abundances_or_none(sample_sig), call_sets)
    if gather_plan is not None:  # one call per chosen coverage on the still-resident database
        from . import residual as _residual  # (the call sets and the sample's abundances are made as for --residual)

        with phases.phase("gather"):
            all_covs = [float(c) for c in (covs if has_raw else covs[1:])]
            all_sets = _residual.call_sets_of(manifest["organism_name"], results if has_raw else results[1:])
            gather_sets = [all_sets[all_covs.index(c)] for c in gather_plan[0]]
            gather_rows = gather.gather_call_sets(hr._LAST_RUN["db"], hr._LAST_RUN["mins"],
                                                  _residual.sample_abundances_or_none(sample_sig), gather_sets, gather_plan[1], gather_cap)
    if lineages is not None:  # one taxonomy and one call on the still-resident database (references in manifest order)
        from . import residual as _residual

        with phases.phase("lca"):
            tree = taxonomy.build_tree(manifest["organism_name"], lineages)
            hr._LAST_RUN["db"].set_taxonomy(*tree[:3])
            lca_abund = _residual.sample_abundances_or_none(sample_sig)
            _, lca_counts = hr._LAST_RUN["db"].lca(hr._LAST_RUN["mins"], lca_abund, want_nodes=False)
            lca_sets = _residual.call_sets_of(manifest["organism_name"], results if has_raw else results[1:])
    hr.release_reference_dbs()
    results = trim_results(results)

    logger.info(f"Saving results to {results_folder}.")
    _t_write = phases.phase("write_results")
    _t_write.__enter__()
    write_sample_results(results, covs, has_raw, results_folder, args.keep_raw, args.show_all)
    if want_abundance:
        abundance.write_profile(results if has_raw else results[1:], covs if has_raw else covs[1:], results_folder)
    if want_residual:
        residual.write_outputs(results_folder, sample_sig, user_covs, call_sets, *explained, residual_cov)
    if gather_plan is not None:
        gather.write_profile(results_folder, sample_sig, gather_plan[0], gather_rows, manifest["organism_name"])
    if lineages is not None:
        n_hashes = len(sample_sig.minhash)
        taxonomy.write_summary(results_folder, taxonomy.summary_frame(
            tree[0], tree[2], tree[3], lca_counts, n_hashes, n_hashes if lca_abund is None else int(sum(int(a) for a in lca_abund)),
            covs if has_raw else covs[1:], lca_sets))
    _t_write.__exit__(None, None, None)


if __name__ == "__main__":
    p = argparse.ArgumentParser(description="Presence/absence of reference organisms in a metagenomic sample.",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    add_arguments(p)
    main(p.parse_args())
