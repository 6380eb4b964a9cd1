"""dge_amd.directions on the GPU, on the 64^2 generator of tests/s2_noise_models.py (its mapping network at checkpoint scale as in
tests/s2z_models.py: otherwise w is of the order 1e-2 and the covariance is degenerate): SeFa and the W-space PCA against their
float64 restatements (tests/directions_ref.py), the command line end to end, and that a fit leaves the launches of a plain
synthesis as they were."""
import numpy as np
import pytest
import torch

from tests import directions_ref as DR
from tests.conftest import meas
from tests.s2_noise_models import S2N_KW, s2n_state_dict
from tests.s2z_models import s2z_state_dict

pytestmark = pytest.mark.gpu

L = 10          # W+ rows of the 64^2 generator: conv block i reads row i (i < 9), toRGB block k reads row 2k + 1 (k < 5)
CLI_MODEL = ["--img_size", "64", "--fmaps_base", "2048", "--fmaps_max", "128", "--compute_dtype", "f32"]


def state_dict():
    sd = s2n_state_dict()
    sd.update({k: v for k, v in s2z_state_dict().items() if k.startswith("mapping.")})
    return sd


@pytest.fixture(scope="module")
def G():
    import dge_amd
    g = dge_amd.StyleGAN2Generator(64, compute_dtype="f32", **S2N_KW).cuda()
    g.load_state_dict(state_dict())
    g.eval()
    return g


@pytest.fixture
def gram_calls(monkeypatch):
    """what every ops.gram call of the test got and gave: (x, mean, row_norm, scale, out)"""
    from dge_amd import ops
    calls, real = [], ops.gram

    def spy(x, mean=None, row_norm=False, scale=1.0):
        out = real(x, mean=mean, row_norm=row_norm, scale=scale)
        calls.append((x, mean, row_norm, scale, out))
        return out
    monkeypatch.setattr(ops, "gram", spy)
    return calls


def blocks_reading(rows):
    """the state-dict names of the blocks that read one of the W+ rows, in the block order of the style codes"""
    return [f"synthesis.layer{i}" for i in range(L - 1) if i in rows] + [f"synthesis.output{k}" for k in range(L // 2) if 2 * k + 1 in rows]


def check_eigen(tag, dirs, M_dev, M64, K):
    """eigenvalues against float64 on M64 within tau(M), residuals and unit norms of every returned direction"""
    M32 = M_dev.cpu().numpy()
    assert np.array_equal(M32, M32.T)
    tau, err = DR.eig_tolerance(M32)
    lam, _ = DR.eigh_ref(M64)
    ev = dirs["eigenvalues"].cpu().numpy().astype(np.float64)
    d = dirs["directions"].cpu().numpy().astype(np.float64)
    assert d.shape == (K, 512) and ev.shape == (K,) and dirs["sigma"].shape == (K,)
    A2 = float(np.abs(lam).max())
    m = dict(tau=tau / (DR.U * A2), evals=np.abs(ev - lam[:K]).max() / (DR.U * A2),
             residual=np.abs(d @ M64 - ev[:, None] * d).max() / (DR.U * A2), norm=np.abs(np.linalg.norm(d, axis=1) - 1).max())
    meas(f"directions.{tag}", **m)
    assert np.abs(ev - lam[:K]).max() <= tau, m
    assert np.abs(d @ M64 - ev[:, None] * d).max() <= tau, m
    assert m["norm"] <= 4 * DR.U, m                                  # 512 components rounded to f32: sqrt(512) 2^-25 at the most
    assert np.all(np.diff(ev) <= 0)
    top = np.argmax(np.abs(d), axis=1)
    assert np.all(d[np.arange(K), top] > 0)
    return tau, lam


@pytest.mark.parametrize("rows,num", [(None, None), ([0, 1, 4], 16), ([4], 3)])
def test_sefa_directions(G, gram_calls, rows, num):
    from dge_amd.directions import sefa_directions
    dirs = sefa_directions(G, rows=rows, num=num)
    sd = state_dict()
    names = blocks_reading(range(L) if rows is None else rows)
    weights = [sd[n + ".style.weight"].numpy() for n in names]
    assert len(names) == {None: 14, 3: 4, 1: 1}[None if rows is None else len(rows)]
    (x, mean, row_norm, scale, M_dev), = gram_calls
    assert x.shape[0] == sum(w.shape[0] for w in weights) and x.shape[1] == 512          # exactly the blocks reading those rows
    assert mean is None and row_norm and scale == 1.0
    assert torch.equal(x.cpu(), torch.cat([torch.from_numpy(w) for w in weights]))
    M64 = DR.sefa_matrix_ref(weights)
    _, bound = DR.gram_ref(np.concatenate(weights), row_norm=True)
    assert np.all(np.abs(M_dev.cpu().numpy().astype(np.float64) - M64) <= bound)
    K = 512 if num is None else num
    check_eigen(f"sefa.rows_{'all' if rows is None else len(rows)}", dirs, M_dev, M64, K)
    assert torch.equal(dirs["sigma"], torch.ones(K, device="cuda")) and dirs["mean"] is None
    assert dirs["method"] == "sefa" and dirs["rows"] == (list(range(L)) if rows is None else rows) and dirs["samples"] is None
    with pytest.raises(ValueError, match="outside the 10 rows"):
        sefa_directions(G, rows=[3, 10])
    with pytest.raises(ValueError, match="num = 513"):
        sefa_directions(G, rows=[4], num=513)


@pytest.mark.parametrize("samples", [64, 1025])
def test_pca_directions(G, gram_calls, samples):
    from dge_amd import ops
    from dge_amd.directions import pca_directions
    dirs = pca_directions(G, samples=samples, seed=5, chunk=500, num=None if samples == 64 else 40)
    (w, mean, row_norm, scale, C_dev), = gram_calls
    assert tuple(w.shape) == (samples, 512) and not row_norm and scale == 1.0 / samples
    # the draws of infer.style_sigma: a CPU generator seeded with `seed`, mapped without truncation
    z = torch.randn(samples, 512, generator=torch.Generator().manual_seed(5))
    first = min(500, samples)                                         # (the first chunk, at its batch size)
    with torch.no_grad():
        assert torch.equal(G.mapping(z[:first].cuda())["w"].float(), w[:first])
    assert torch.equal(mean, ops.cols_mean_std(w)[0]) and torch.equal(dirs["mean"], mean)
    assert float(w.std()) > 0.1                                       # checkpoint scale: the covariance is far above rounding
    wh, mh = w.cpu().numpy(), mean.cpu().numpy()
    C64, bound = DR.gram_ref(wh, mean=mh, scale=float(np.float32(1.0 / samples)))
    assert np.all(np.abs(C_dev.cpu().numpy().astype(np.float64) - C64) <= bound)
    K = 512 if samples == 64 else 40
    tau, lam = check_eigen(f"pca.{samples}", dirs, C_dev, DR.pca_matrix_ref(wh, mh), K)
    ev, sigma = dirs["eigenvalues"].cpu().double(), dirs["sigma"].cpu().double()
    assert torch.isfinite(sigma).all() and (sigma >= 0).all()
    assert torch.all((sigma * sigma - ev.clamp(min=0)).abs() <= 2.0 ** -22 * ev.clamp(min=0))          # sigma^2 = max(eval, 0), f32 sqrt
    if samples == 64:                                                 # centred rows: rank <= 63
        assert float(ev[63:].abs().max()) <= tau
        assert torch.all(sigma[ev <= 0] == 0)
    assert dirs["method"] == "pca" and dirs["samples"] == samples and dirs["seed"] == 5 and dirs["rows"] == list(range(L))


def tiles(path, n, S=64):
    """the n tiles of a one-row save_image_grid PNG (2 px padding) as uint8 [S,S,3]"""
    from PIL import Image
    img = np.asarray(Image.open(path).convert("RGB"))
    assert img.shape == (S + 4, n * (S + 2) + 2, 3)
    return [img[2:2 + S, 2 + i * (S + 2):2 + i * (S + 2) + S] for i in range(n)]


def test_cli_fit_and_apply(G, tmp_path):
    from PIL import Image
    from dge_amd import directions, ops
    from dge_amd.infer import quantize_u8
    from dge_amd.projector import main as projector_main
    ckpt = str(tmp_path / "g.pt")
    torch.save({"generator_smooth": state_dict()}, ckpt)
    model = CLI_MODEL + ["--checkpoint_dir_GAN", ckpt]
    paths = {m: str(tmp_path / f"{m}.pt") for m in ("sefa", "pca")}
    directions.main(["fit", "--method", "sefa", "--rows", "0-5", "--num", "8", "--out", paths["sefa"]] + model)
    directions.main(["fit", "--method", "pca", "--samples", "200", "--seed", "3", "--num", "6", "--out", paths["pca"]] + model)
    sefa, pca = directions.load_directions(paths["sefa"]), directions.load_directions(paths["pca"])
    assert tuple(sefa["directions"].shape) == (8, 512) and sefa["rows"] == [0, 1, 2, 3, 4, 5] and not sefa["directions"].is_cuda
    assert tuple(pca["directions"].shape) == (6, 512) and pca["samples"] == 200 and pca["seed"] == 3 and tuple(pca["mean"].shape) == (512,)
    want = directions.pca_directions(G, samples=200, seed=3, num=6)
    assert torch.equal(want["directions"].cpu(), pca["directions"]) and torch.equal(want["sigma"].cpu(), pca["sigma"])
    # apply without noise maps: tile 0 is the unedited code's image, tile 1 moved
    wp = torch.randn(1, L, 512, generator=torch.Generator().manual_seed(9))
    torch.save(wp, tmp_path / "wp.pt")
    strip = str(tmp_path / "strip.png")
    directions.main(["apply", "--directions", paths["pca"], "--wp", str(tmp_path / "wp.pt"), "--index", "1", "--amounts", "0,2", "--rows", "0-8",
                     "--out", strip] + model)
    t0, t1 = tiles(strip, 2)
    with torch.no_grad():
        q = quantize_u8(G.synthesis(wp.cuda())["image"])[0].cpu().numpy()
        moved = directions.edit_direction(wp.cuda(), pca, 1, 2.0, start=0, end=9)
        q1 = quantize_u8(G.synthesis(moved)["image"])[0].cpu().numpy()
    assert np.array_equal(t0, q) and np.array_equal(t1, q1) and not np.array_equal(t0, t1)
    assert torch.equal(moved[0, 9], wp[0, 9].cuda()) and not torch.equal(moved[0, 8], wp[0, 8].cuda())          # --rows 0-8
    # with the noise maps of a two-step projector run, amount 0 reproduces the run's rec PNG
    torch.save(torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(5)), tmp_path / "imgs.pt")
    out = tmp_path / "proj"
    was = ops.is_deterministic()
    try:
        projector_main(["--steps", "2", "--allow_standin_lpips", "--w_avg_samples", "64", "--save_every", "1", "--launch", "eager",
                        "--img_dir", str(tmp_path / "imgs.pt"), "--experiment_dir", str(out)] + model)
    finally:
        ops.set_deterministic(was)
    strip2 = str(tmp_path / "strip2.png")
    directions.main(["apply", "--directions", paths["sefa"], "--wp", str(out / "models" / "id0-wp.pt"), "--noise", str(out / "models" / "id0-noise.pt"),
                     "--index", "7", "--amounts", "0,3", "--out", strip2] + model)
    r0, r1 = tiles(strip2, 2)
    rec = np.asarray(Image.open(out / "rec" / "00000.png").convert("RGB"))
    assert np.array_equal(r0, rec) and not np.array_equal(r1, rec)
    with pytest.raises(SystemExit, match="holds"):
        directions.main(["apply", "--directions", paths["sefa"], "--wp", str(out / "models" / "id0-w.pt"), "--out", strip2] + model)


def test_fit_leaves_the_launches_of_synthesis_alone(G):
    from dge_amd import ops
    from dge_amd.directions import pca_directions, sefa_directions
    wp = torch.randn(1, L, 512, generator=torch.Generator().manual_seed(2)).cuda()

    def logged():          # KERNEL_LOG and the conv-family launches (ops.PROFILE's shape tags: at 64^2 the forward logs nothing else)
        ops.KERNEL_LOG, ops.PROFILE = log, prof = [], []
        try:
            with torch.no_grad():
                img = G.synthesis(wp)["image"].clone()
            return ([(n, s.value) for n, s in log], [e[3] for e in prof]), img
        finally:
            ops.KERNEL_LOG = ops.PROFILE = None
    before, img0 = logged()
    ops.KERNEL_LOG = []
    try:
        sefa_directions(G, num=4)
        pca_directions(G, samples=64, num=4)
        fit_log = [n for n, _ in ops.KERNEL_LOG]
    finally:
        ops.KERNEL_LOG = None
    after, img1 = logged()
    assert before[1] and before == after and torch.equal(img0, img1)
    assert fit_log.count("gram") == 2 and fit_log.count("eigh_sym") == 2 and "cols_mean_std" in fit_log
