"""`python -m dge_amd.mis_align`: the parser (defaults of the three scripts, refusals) without a GPU, and on the GPU a three-iteration
run of case 2 that writes the scripts' dump files."""
import os

import pytest

from dge_amd import mis_align as M


@pytest.mark.parametrize("case,iterations,batch", [("s1", 210000, 5), ("1", 120001, 8), ("2", 120001, 8)])
def test_parser_defaults_follow_the_scripts(case, iterations, batch):
    args = M.parse_args([] if case == "s1" else ["--case", case])       # (s1 is the default case)
    assert args.case == case
    assert (args.iterations, args.batch_size, args.img_size, args.start_features, args.mtype) == (iterations, batch, 256, 64, 2)
    assert (args.lr, args.beta_1, args.z_dim) == (0.0015, 0.0, 512)
    assert args.attention == "pair" and not args.legacy_zero_grad and args.vgg16_weights is None
    assert args.experiment_dir is None and not args.deterministic and not args.allow_standin_lpips


def test_explicit_flags_override_the_case_defaults():
    args = M.parse_args(["--batch_size", "3", "--case", "2", "--iterations", "7", "--attention", "fused", "--legacy_zero_grad",
                         "--mtype", "1"])
    assert (args.case, args.batch_size, args.iterations, args.attention, args.legacy_zero_grad, args.mtype) == ("2", 3, 7, "fused", True, 1)


def test_bad_case_is_rejected(capsys):
    with pytest.raises(SystemExit) as e:
        M.parse_args(["--case", "3"])
    assert e.value.code == 2 and "--case" in capsys.readouterr().err


def test_more_than_one_process_is_rejected(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        M.parse_args(["--case", "2"])
    assert "more than one process is not offered" in str(e.value)


@pytest.mark.parametrize("case", ["1", "2"])
@pytest.mark.parametrize("mtype", ["3", "4"])
def test_cases_1_and_2_reject_pggan_and_biggan(case, mtype):
    with pytest.raises(SystemExit) as e:
        M.parse_args(["--case", case, "--mtype", mtype])
    assert "loss_c is not meaningful" in str(e.value)
    assert M.parse_args(["--case", "s1", "--mtype", mtype]).mtype == int(mtype)          # the s1 script handles all four


def test_new_entry_points_are_bound():
    from dge_amd import _lib
    for name in ("dge_class_target_groups", "dge_gather_row_groups", "dge_mask2cam_groups", "dge_minmax_unit", "dge_minmax_unit_slots"):
        assert name in _lib.SIGNATURES


@pytest.mark.gpu
def test_three_iteration_run_writes_the_dump_files(tmp_path, capsys):
    from PIL import Image
    out = str(tmp_path / "run")
    args = M.parse_args(["--case", "2", "--iterations", "3", "--img_size", "64", "--fmaps_base", "2048", "--fmaps_max", "128",
                         "--enc_maxf", "64", "--start_features", "16", "--batch_size", "2", "--allow_standin_lpips",
                         "--experiment_dir", out])
    st = M.train(None, args, dump_every=2, save_every=2)
    assert (st.case, st.attention) == ("case2", "pair")
    assert "seeded stand-in VGG16" in capsys.readouterr().out
    want = ["imgs/ep0_iter%d.png", "grad_cam/heatmap_%d.png", "grad_cam/cam_%d.png", "grad_cam/gb_%d.png", "models/E_model_ep0_iter%d.pth"]
    for it in (0, 2):
        for f in want:
            assert os.path.getsize(os.path.join(out, f % it)) > 0, f % it
    for f in want:
        assert not os.path.exists(os.path.join(out, f % 1))
    # two rows of two 64 x 64 images, 2 px padding: imgs1 over imgs2
    for f in ("imgs/ep0_iter2.png", "grad_cam/gb_2.png"):
        assert Image.open(os.path.join(out, f)).size == (2 * 66 + 2, 2 * 66 + 2)
    gb = Image.open(os.path.join(out, "grad_cam/gb_2.png"))
    lo, hi = zip(*gb.getextrema())
    assert min(lo) == 0 and max(hi) == 255              # min-max normalised over the whole [2N,3,H,W] array
    txt = open(os.path.join(out, "Loss.txt")).read()
    assert txt.count("---------ImageSpace--------") == 2 and "i_0\n" in txt and "i_2\n" in txt and "i_1\n" not in txt
    for tag in ("mask", "grad", "imgs", "Gcam", "w", "c"):
        assert txt.count("loss_%s_info: " % tag) == 2
    assert "loss_c_info: None" in txt                    # enc_maxf 64 against fmaps_max 128: the logged loss_c cannot be formed
