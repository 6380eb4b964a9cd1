"""Command line of the independent-rows BigGAN-deep inversion (dge_amd.embedding_v2_biggan --independent / --labels): defaults, strict
parsing, the refusals, the two --labels forms and the padded last group.  No GPU."""
import pytest


def test_defaults_are_unchanged():
    from dge_amd.embedding_v2_biggan import parse_args
    a = parse_args([])
    assert a.independent is False and a.labels is None and a.optimizeE is True and a.label == 30 and a.batch_size == 1
    a = parse_args(["--optimizeE", "false"])
    assert a.independent is False and a.labels is None


def test_independent_parses_strictly():
    from dge_amd.embedding_v2_biggan import parse_args
    for v, want in (("true", True), ("True", True), ("false", False), ("0", False)):
        assert parse_args(["--optimizeE", "false", "--independent", v]).independent is want
    for bad in ("maybe", "", "2"):
        with pytest.raises(SystemExit):
            parse_args(["--optimizeE", "false", "--independent", bad])


def test_independent_needs_the_frozen_encoder():
    from dge_amd.embedding_v2_biggan import parse_args
    with pytest.raises(SystemExit, match="--independent true needs --optimizeE false"):
        parse_args(["--independent", "true", "--optimizeE", "true"])
    with pytest.raises(SystemExit, match="--independent true needs --optimizeE false"):
        parse_args(["--independent", "true"])          # --optimizeE defaults to true
    a = parse_args(["--independent", "true", "--optimizeE", "false", "--batch_size", "4", "--labels", "30,207,5,1,9"])
    assert a.independent is True and a.labels == "30,207,5,1,9" and a.batch_size == 4


def test_labels_need_independent():
    from dge_amd.embedding_v2_biggan import parse_args
    with pytest.raises(SystemExit, match="--labels needs --independent true"):
        parse_args(["--optimizeE", "false", "--labels", "30,207"])
    with pytest.raises(SystemExit, match="--labels needs --independent true"):
        parse_args(["--optimizeE", "false", "--independent", "false", "--labels", "30,207"])


def test_labels_wrong_length_and_out_of_range_exit():
    from dge_amd.embedding_v2_biggan import read_labels
    assert read_labels(None, 3, 1000, 30) == [30, 30, 30]
    assert read_labels("30,207,5", 3, 1000, 30) == [30, 207, 5]
    with pytest.raises(SystemExit, match="2 class ids for 3 images"):
        read_labels("30,207", 3, 1000, 30)
    with pytest.raises(SystemExit, match="4 class ids for 3 images"):
        read_labels("30,207,5,1", 3, 1000, 30)
    with pytest.raises(SystemExit, match="outside"):
        read_labels("30,1000,5", 3, 1000, 30)
    with pytest.raises(SystemExit, match="outside"):
        read_labels("30,-1,5", 3, 1000, 30)
    with pytest.raises(SystemExit, match="integer class ids"):
        read_labels("30,frog,5", 3, 1000, 30)


def test_file_and_comma_forms_agree(tmp_path):
    from dge_amd.embedding_v2_biggan import read_labels
    f = tmp_path / "labels.txt"
    f.write_text("30\n207\n5\n1\n9\n")
    assert read_labels(str(f), 5, 1000, 30) == read_labels("30,207,5,1,9", 5, 1000, 30) == [30, 207, 5, 1, 9]
    with pytest.raises(SystemExit, match="5 class ids for 4 images"):
        read_labels(str(f), 4, 1000, 30)


def test_padded_last_group_repeats_image_and_label():
    from dge_amd.embedding_v2_biggan import rows_plan
    plan = rows_plan(5, 4, [30, 207, 5, 1, 9])
    assert plan == [(0, 4, [0, 1, 2, 3], [30, 207, 5, 1]), (4, 1, [4, 4, 4, 4], [9, 9, 9, 9])]
    assert rows_plan(4, 2, [1, 2, 3, 4]) == [(0, 2, [0, 1], [1, 2]), (2, 2, [2, 3], [3, 4])]
    assert sum(keep for _, keep, _, _ in plan) == 5          # every image once; the padded rows are dropped by `keep`


def test_rows_step_refuses_mode_e_without_a_gpu():
    from dge_amd import embedding_v2_biggan as M
    assert issubclass(M.BigEmbedRowsStep, M.BigEmbedStep) and M.BigEmbedRowsStep.independent is True
    with pytest.raises(ValueError, match="mode 'W' only"):
        M.BigEmbedRowsStep(None, None, None, mode="E")
