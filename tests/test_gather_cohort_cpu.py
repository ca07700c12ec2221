"""`yacht run --gather --gather_top K`, the parts that need no device: parsing and validation of the option -- alone, below 1,
above the cohort's maximum, and a cohort without it -- all before anything is written, the cap reaching the single sample's
ranking, the batch binding's own argument checks, and the long-form frame of results/cohort_gather.tsv from hand-made rows."""
import argparse
import os

import numpy as np
import pytest

from yacht_amd import _lib, engine, gather, run_YACHT

HERE = os.path.dirname(os.path.abspath(__file__))


def _parse(*argv, files=("a.sig.zip",)):
    p = argparse.ArgumentParser()
    run_YACHT.add_arguments(p)
    return p.parse_args(["--json", "x.json", "--sample_file", *files, *argv])


def test_abi_and_binding_name_the_batch_entry():
    with open(os.path.join(HERE, "..", "include", "yacht_hip.h")) as f:
        text = f.read()
    assert "int yh_gather_batch_device(" in text and "int yh_gather_batch(" in text and "#define YH_ABI_VERSION 8" in text
    assert "#define YH_GATHER_BATCH_MAX_ROWS 4096" in text
    assert "yh_gather_batch / yh_gather_batch_device" in text  # its row of the interleaving table
    assert len(_lib.SIGNATURES["yh_gather_batch_device"][1]) == 14 and len(_lib.SIGNATURES["yh_gather_batch"][1]) == 13
    assert _lib.YH_GATHER_BATCH_MAX_ROWS == 4096 == gather.TOP_MAX_COHORT


def test_parser_takes_the_option_with_its_default():
    args = _parse()
    assert args.gather_top is None and gather.gather_top(args) is None and gather.gather_options(args) is None
    args = _parse("--gather", "--gather_top", "50")
    assert args.gather_top == 50 and gather.gather_top(args) == 50
    assert gather.gather_options(args) == ([1.0, 0.5, 0.1, 0.05, 0.01], 1)  # (the plan keeps its shape: the cap is read on its own)
    # one sample file may ask for more than a cohort's maximum; a cohort may ask for exactly that
    assert gather.gather_top(_parse("--gather", "--gather_top", "100000")) == 100000
    two = ("a.sig.zip", "b.sig.zip")
    args = _parse("--gather", "--gather_top", str(gather.TOP_MAX_COHORT), "--gather_min_hits", "3", "--gather_coverage", "0.1", files=two)
    assert gather.gather_top(args, 2) == gather.TOP_MAX_COHORT and gather.gather_options(args, 2) == ([0.1], 3)


@pytest.mark.parametrize("argv,files,message", [
    (["--gather_top", "5"], 1, "--gather_top needs --gather"),
    (["--gather_top", "5"], 2, "--gather_top needs --gather"),
    (["--gather", "--gather_top", "0"], 1, "at least 1, not 0"),
    (["--gather", "--gather_top", "-3"], 2, "at least 1, not -3"),
    (["--gather", "--gather_top", "4097"], 2, "at most 4096 for a cohort, not 4097"),
    (["--gather"], 2, "one sample file, not 2"),
    (["--gather", "--gather_coverage", "0.1"], 3, "one sample file, not 3"),
])
def test_refusals_come_before_any_work(tmp_path, argv, files, message):
    names = tuple(f"s{i}.sig.zip" for i in range(files))
    args = _parse(*argv, "--outdir", str(tmp_path / "out"), files=names)
    with pytest.raises(ValueError, match=message):
        gather.gather_options(args, files)
    # through the command's main: nothing is read (neither the config nor the samples exist) and nothing is written
    with pytest.raises(ValueError, match=message):
        run_YACHT.main(args)
    assert not (tmp_path / "out").exists() and os.listdir(tmp_path) == []


def test_the_cohort_message_names_the_option():
    with pytest.raises(ValueError) as ei:
        gather.gather_options(_parse("--gather", files=("a.sig.zip", "b.sig.zip")), 2)
    text = str(ei.value)
    assert text.startswith("--gather takes one sample file, not 2") and "--gather_top" in text and "4096" in text


def test_the_cap_reaches_the_single_samples_ranking():
    class Db:
        n_refs = 4
        calls = []

        def gather(self, sample, cand, abund, min_hits, cap_rows):
            self.calls.append((cand.tolist(), min_hits, cap_rows))
            return np.zeros(0, engine.GATHER_ROW_DTYPE), False, None

    db = Db()
    gather.gather_call_sets(db, np.zeros(0, np.uint64), None, [[1, 2], [3]], 2, 50)
    gather.gather_call_sets(db, np.zeros(0, np.uint64), None, [[0]])
    assert db.calls == [([0, 1, 1, 0], 2, 50), ([0, 0, 0, 1], 2, 50), ([1, 0, 0, 0], 1, None)]


def test_batch_binding_checks_its_limits_on_the_host():
    assert engine.check_gather_batch_limits(1, 1, None, 9) == (1, 1, 9)
    assert engine.check_gather_batch_limits(0x40, 3, 4, 9) == (0x40, 3, 4) and engine.check_gather_batch_limits(255, 1, 0, 9) == (255, 1, 0)
    assert engine.check_gather_batch_limits(1, 1, None, 100_000) == (1, 1, 4096) and engine.check_gather_batch_limits(1, 1, 4096, 100_000) == (1, 1, 4096)
    for bad in (0, 256, -1, 1.5):
        with pytest.raises(ValueError, match="cand_mask"):
            engine.check_gather_batch_limits(bad, 1, None, 9)
    for bad in (4097, -1, 2.5):
        with pytest.raises(ValueError, match="cap_rows"):
            engine.check_gather_batch_limits(1, 1, bad, 9)
    for bad in (0, 2 ** 32):
        with pytest.raises(ValueError, match="min_hits"):
            engine.check_gather_batch_limits(1, bad, None, 9)


def _rows(*rows):
    out = np.zeros(len(rows), dtype=engine.GATHER_ROW_DTYPE)
    for k, (ref, n_ov, n_un, w) in enumerate(rows):
        out[k] = (ref, n_ov, n_un, 0, w)
    return out


def test_long_form_frame_from_hand_made_rows(tmp_path):
    names = ["org_a", "org_b", "org_c"]
    first = gather.gather_frame([1.0, 0.1], [_rows((2, 50, 50, 400)), _rows((2, 50, 50, 400), (0, 40, 10, 25))], names, 200, 1000)
    none = gather.gather_frame([1.0, 0.1], [_rows(), _rows()], names, 10, 10)
    third = gather.gather_frame([1.0, 0.1], [_rows(), _rows((1, 7, 7, 7))], names, 70, 70)
    frame = gather.cohort_frame(["s1", "s2", "s3"], [first, none, third])
    assert list(frame.columns) == ["sample"] + gather.GATHER_COLUMNS
    assert frame["sample"].tolist() == ["s1", "s1", "s1", "s3"]  # a sample without rows has none here either
    assert frame["min_coverage"].tolist() == [1.0, 0.1, 0.1, 0.1] and frame["rank"].tolist() == [0, 0, 1, 0]
    assert frame["organism_name"].tolist() == ["org_c", "org_c", "org_a", "org_b"]
    assert frame["num_unique"].tolist() == [50, 50, 10, 7] and frame["f_unique_of_sample"].tolist() == [0.25, 0.25, 0.05, 0.1]
    # the same rows as the samples' own files, behind the sample column
    for stem, own in (("s1", first), ("s3", third)):
        part = frame[frame["sample"] == stem].drop(columns="sample").reset_index(drop=True)
        assert part.astype(str).equals(own.astype(str))
    assert len(first) == 3  # (cohort_frame copies: the sample's own frame is not changed)
    assert "sample" not in first.columns
    empty = gather.cohort_frame([], [])
    assert list(empty.columns) == ["sample"] + gather.GATHER_COLUMNS and len(empty) == 0
    assert len(gather.cohort_frame(["s2"], [none])) == 0
    # write_frame writes what write_profile would
    gather.write_frame(str(tmp_path), first)
    text = (tmp_path / gather.GATHER_NAME).read_text()
    assert text.splitlines()[0].split("\t") == gather.GATHER_COLUMNS and len(text.splitlines()) == 4
