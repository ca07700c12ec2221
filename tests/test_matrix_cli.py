"""`yacht run --matrix`: every combination the command refuses, against its MSG_* text, before any device work and with
nothing written.  No GPU."""
import json
import os

import numpy as np
import pytest

from yacht_amd import cli, cohort, matrix, run_YACHT, sigio


@pytest.fixture
def setup(tmp_path, monkeypatch):
    """A config + manifest as `yacht train` leaves them, two samples, an output directory, and a guard that fails on device work."""
    work = tmp_path / "db_intermediate_files"
    work.mkdir()
    manifest = tmp_path / "db_processed_manifest.tsv"
    manifest.write_text("organism_name\tmd5sum\tnum_unique_kmers_in_genome_sketch\tnum_total_kmers_in_genome_sketch\t"
                        "genome_scale_factor\norg\t0123\t10\t10\t1000\n")
    cfg = tmp_path / "db_config.json"
    cfg.write_text(json.dumps({"manifest_file_path": str(manifest), "intermediate_files_dir": str(work), "scale": 1000,
                               "ksize": 31, "ani_thresh": 0.95}))
    out = tmp_path / "out"
    out.mkdir()
    files = []
    for i in range(2):
        rng = np.random.default_rng(i)
        mins = np.unique(rng.integers(0, sigio.max_hash_for_scaled(1000), 200, dtype=np.uint64))
        files.append(tmp_path / f"s{i}.sig.zip")
        sigio.write_sig_zip([sigio.make_signature(mins, ksize=31, scaled=1000, name=f"s{i}", abundances=np.ones(mins.size, dtype=np.int64))],
                            str(files[-1]))

    def no_device(*a, **k):
        raise AssertionError("device work started before every input was checked")

    monkeypatch.setattr(cohort.hr, "get_reference_db", no_device)
    monkeypatch.setattr(run_YACHT.hr, "hypothesis_recovery", no_device)
    monkeypatch.setattr(cohort, "_Device", no_device)
    monkeypatch.delenv(matrix.ENV, raising=False)
    return cfg, out, files


def _argv(cfg, out, files, *opts):
    return ["run", "--json", str(cfg), "--sample_file", *map(str, files), "--num_threads", "2", "--outdir", str(out), *opts]


def _refused(cfg, out, files, opts, message):
    with pytest.raises(ValueError) as ei:
        cli.main(_argv(cfg, out, files, *opts))
    assert str(ei.value) == message
    assert os.listdir(out) == []  # nothing written
    if len(files) > 1:  # the cohort's own check refuses it too
        args = cli.build_parser().parse_args(_argv(cfg, out, files, *opts))
        with pytest.raises(ValueError) as ei:
            cohort.check_inputs(args, [str(f) for f in files])
        assert str(ei.value) == message


def test_parser_and_defaults():
    flags = [f for f, _ in run_YACHT.ARGUMENTS]
    assert {"--matrix", "--matrix_coverage", "--matrix_min_samples"} <= set(flags)
    args = cli.build_parser().parse_args(["run", "--json", "c", "--sample_file", "a", "b", "--matrix"])
    assert args.matrix is True and args.matrix_coverage is None and args.matrix_min_samples is None
    assert matrix.matrix_options(args, 2) == (0.01, 1, False)  # the smallest of the default list, as --residual_coverage
    plain = cli.build_parser().parse_args(["run", "--json", "c", "--sample_file", "a", "b"])
    assert plain.matrix is False and matrix.matrix_options(plain, 2) is None
    args = cli.build_parser().parse_args(["run", "--json", "c", "--sample_file", "a", "b", "--matrix", "--min_coverage_list", "0.5", "0.1", "0.5",
                                          "--matrix_coverage", "0.5", "--matrix_min_samples", "3"])
    assert matrix.matrix_options(args, 2) == (0.5, 3, False)


def test_one_file_is_refused(setup):
    cfg, out, files = setup
    _refused(cfg, out, files[:1], ["--matrix"], matrix.MSG_MATRIX_NEEDS_COHORT.format(1))


def test_unlisted_coverage_is_refused(setup):
    cfg, out, files = setup
    _refused(cfg, out, files, ["--matrix", "--min_coverage_list", "1", "0.1", "--matrix_coverage", "0.5"],
             matrix.MSG_COVERAGE_NOT_LISTED.format(0.5, [1.0, 0.1]))


def test_coverage_without_the_flag_is_refused(setup):
    cfg, out, files = setup
    _refused(cfg, out, files, ["--matrix_coverage", "0.1"], matrix.MSG_COVERAGE_WITHOUT_MATRIX)
    _refused(cfg, out, files[:1], ["--matrix_coverage", "0.1"], matrix.MSG_COVERAGE_WITHOUT_MATRIX)


def test_min_samples_is_checked(setup):
    cfg, out, files = setup
    _refused(cfg, out, files, ["--matrix", "--matrix_min_samples", "0"], matrix.MSG_BAD_MIN_SAMPLES.format(0))
    _refused(cfg, out, files, ["--matrix", "--matrix_min_samples", "-2"], matrix.MSG_BAD_MIN_SAMPLES.format(-2))
    _refused(cfg, out, files, ["--matrix_min_samples", "2"], matrix.MSG_MIN_SAMPLES_WITHOUT_MATRIX)


def test_33_coverages_are_refused(setup):
    cfg, out, files = setup
    covs = [str((i + 1) / 40) for i in range(33)]
    _refused(cfg, out, files, ["--matrix", "--min_coverage_list", *covs], matrix.MSG_TOO_MANY_COVERAGES.format(33))
    args = cli.build_parser().parse_args(_argv(cfg, out, files, "--matrix", "--min_coverage_list", *covs[:32]))
    assert matrix.matrix_options(args, 2) == (1 / 40, 1, False)  # 32 fit the mask
    args = cli.build_parser().parse_args(_argv(cfg, out, files, "--min_coverage_list", *covs))
    assert matrix.matrix_options(args, 2) is None  # (without the flag the list is not its business)


def test_a_bad_route_word_is_refused(setup, monkeypatch):
    cfg, out, files = setup
    monkeypatch.setenv(matrix.ENV, "numpy")
    _refused(cfg, out, files, ["--matrix"], matrix.MSG_BAD_ROUTE.format("numpy"))
    monkeypatch.setenv(matrix.ENV, "host")
    args = cli.build_parser().parse_args(_argv(cfg, out, files, "--matrix"))
    assert matrix.matrix_options(args, 2) == (0.01, 1, True)
    with pytest.raises(AssertionError, match="device work"):  # accepted: the run goes on to the (guarded) database
        cli.main(_argv(cfg, out, files, "--matrix"))
