"""Command line of the independent inversion mode (dge_amd.embedding_v2 --independent): flag parsing, the refusal together with
encoder fine-tuning, and the grouping of a folder into padded batches.  No GPU."""
import pytest


def test_independent_flag_parses_strictly_and_defaults_to_false():
    from dge_amd.embedding_v2 import parse_args
    assert parse_args([]).independent is False
    assert parse_args(["--optimizeE", "false"]).independent is False
    assert parse_args(["--optimizeE", "false", "--independent", "true"]).independent is True
    assert parse_args(["--optimizeE", "false", "--independent", "false"]).independent is False
    with pytest.raises(SystemExit):
        parse_args(["--optimizeE", "false", "--independent", "maybe"])
    with pytest.raises(SystemExit):
        parse_args(["--optimizeE", "false", "--independent"])


def test_independent_with_encoder_fine_tuning_exits_with_a_message():
    from dge_amd.embedding_v2 import parse_args
    for argv in (["--independent", "true", "--optimizeE", "true"], ["--independent", "true"], ["--mtype", "2", "--independent", "true"]):
        with pytest.raises(SystemExit) as e:
            parse_args(argv)
        assert "--independent" in str(e.value) and "--optimizeE false" in str(e.value)


def test_group_plan_and_padding():
    from dge_amd.embedding_v2 import group_plan, padded_rows
    plan = group_plan(5, 2)
    assert plan == [(0, 2), (2, 2), (4, 1)]                                   # 3 groups, the last keeps one row
    rows = [padded_rows(first, 2, 5) for first, _ in plan]
    assert rows == [[0, 1], [2, 3], [4, 4]]                                   # the short group repeats its last image
    kept = [num for (first, keep), r in zip(plan, rows) for num in r[:keep]]
    assert kept == [0, 1, 2, 3, 4]                                            # image numbers 0-4, one padded row dropped
    assert sum(len(r) - keep for (_, keep), r in zip(plan, rows)) == 1
    assert group_plan(6, 4) == [(0, 4), (4, 2)] and padded_rows(4, 4, 6) == [4, 5, 5, 5]
    assert group_plan(4, 4) == [(0, 4)] and group_plan(0, 4) == []


def test_independent_step_needs_w_mode():
    from dge_amd.embedding_v2 import LatentEmbedStep
    with pytest.raises(ValueError, match="independent"):
        LatentEmbedStep(None, None, None, mode="E", generator="sg2", independent=True)


class _StubEncoder:
    """What begin_image needs of an encoder in W mode with a StyleGAN2 generator: the number of W+ rows."""
    layer_count = 5

    def parameters(self):
        return []

    def eval(self):
        return self


def test_independent_start_codes_are_the_batch_one_draws_of_the_image_numbers():
    """Row b of group g starts from randn(1, L, 512) under manual_seed(seed + g*B + b): the code a batch-1 run (coupled path, seed +
    group) draws for image number g*B + b.  `group` advances once per begin_image, which the file numbering g*B + b relies on."""
    import torch
    from dge_amd.embedding_v2 import LatentEmbedStep
    B, seed = 2, 7
    ind = LatentEmbedStep(None, _StubEncoder(), None, mode="W", generator="sg2", seed=seed, independent=True)
    one = LatentEmbedStep(None, _StubEncoder(), None, mode="W", generator="sg2", seed=seed)
    imgs = torch.zeros(B, 3, 8, 8)
    for g in range(3):
        ind.begin_image(imgs)
        assert ind.group == g and tuple(ind.w1.shape) == (B, 10, 512)
        for b in range(B):
            one.begin_image(imgs[:1])
            assert one.group == g * B + b
            want = torch.randn((1, 10, 512), generator=torch.Generator().manual_seed(seed + g * B + b))
            assert torch.equal(ind.w1.detach()[b:b + 1], want) and torch.equal(one.w1.detach(), want)
    for tr in ind.tracker():                                  # every row's minima restart with the group
        assert (tr["min_loss"], tr["min_norm"]) == (100.0, 1000.0) and tr["iteration"] == 0 and tr["events"] == []
