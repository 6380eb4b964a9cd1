"""CPU side of the StyleSpace codes: style_codes.StyleCodes' layout against the arithmetic of autograd_s2._style_tables stated on
its own (block g of batch B at B * off_g, conv blocks first), the file format round trip, infer.edit_styles on CPU tensors, the
layering of the new module and the C ABI's new declarations."""
import os
import subprocess
import sys

import pytest
import torch

from tests.conftest import ROOT
from tests.s2_noise_models import S2N_KW
from tests.s2_style_models import S64_CHANNELS, S64_NAMES, S64_ROWS


def synthesis():
    from dge_amd.stylegan2_generator import SynthesisModule
    return SynthesisModule(64, compute_dtype="f32", **S2N_KW)


@pytest.mark.parametrize("B", [1, 3])
def test_layout_offsets_and_views(B):
    from dge_amd.autograd_s2 import style_groups
    from dge_amd.style_codes import StyleCodes, style_layout
    syn = synthesis()
    c = StyleCodes(syn, B, "cpu")
    assert tuple(c.names) == S64_NAMES and tuple(c.channels) == S64_CHANNELS
    assert tuple(row for _, row in style_groups(syn)) == S64_ROWS          # the row of wp that drives each block
    off, want = 0, []
    for C in S64_CHANNELS:          # _style_tables: s_off.append(B * off); off += C;  s_total = B * off
        want.append(B * off)
        off += C
    assert c.offsets == want and c.numel == B * off == c.flat.numel() == c.grads.numel()
    assert style_layout(syn, B) == (list(S64_NAMES), list(S64_CHANNELS), want, B * off)
    assert c.flat.requires_grad and c.flat.is_leaf and c.flat.dtype == torch.float32 and not c.grads.requires_grad
    # the views sit on the flat storage: element (b, ch) of block g is flat[B * off_g + b * C_g + ch]
    with torch.no_grad():
        c.flat.copy_(torch.arange(c.numel, dtype=torch.float32))
        c.grads.copy_(-torch.arange(c.numel, dtype=torch.float32))
    for g, (blk, gv, C) in enumerate(zip(c.blocks, c.grad_blocks, S64_CHANNELS)):
        assert tuple(blk.shape) == (B, C) == tuple(gv.shape) and not blk.requires_grad
        for b, ch in ((0, 0), (B - 1, C - 1), (B // 2, C // 3)):
            assert float(blk[b, ch]) == want[g] + b * C + ch == -float(gv[b, ch])
    assert c.detached().data_ptr() == c.flat.data_ptr() and not c.detached().requires_grad
    assert c.index("layer0") == 0 and c.index("output0") == 9 and c.index(-1) == 13 and c.index("output4") == 13
    with pytest.raises(ValueError, match="no block"):
        c.index("layer9")
    assert c.fits(B, "cpu") and not c.fits(B + 1, "cpu")


def test_rows_round_trip_is_the_file_format(tmp_path):
    from dge_amd.style_codes import StyleCodes, save_style_rows
    syn = synthesis()
    c = StyleCodes(syn, 3, "cpu")
    with torch.no_grad():
        c.flat.copy_(torch.randn(c.numel, generator=torch.Generator().manual_seed(1)))
    rows = c.rows(1)
    assert [tuple(r.shape) for r in rows] == [(1, C) for C in S64_CHANNELS]
    assert all(torch.equal(r[0], blk[1]) for r, blk in zip(rows, c.blocks))
    rows[0][0, 0] = 123.0          # a copy: the codes do not move
    assert float(c.blocks[0][1, 0]) != 123.0
    save_style_rows(c, [1, 2], [7, 9], str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["id7-s.pt", "id9-s.pt"]
    d = StyleCodes(syn, 2, "cpu")
    d.load_rows(0, torch.load(tmp_path / "id9-s.pt"))
    d.load_rows(1, torch.load(tmp_path / "id7-s.pt"))
    for blk3, blk2 in zip(c.blocks, d.blocks):
        assert torch.equal(blk2[0], blk3[2]) and torch.equal(blk2[1], blk3[1])
    with pytest.raises(ValueError, match="a list of 14 tensors"):
        d.load_rows(0, rows[:-1])
    with pytest.raises(ValueError, match=r"block 3 must be a tensor \[1,128\]"):
        d.load_rows(0, [r if g != 3 else r[:, :5] for g, r in enumerate(rows)])
    with pytest.raises(ValueError, match="outside the 2 rows"):
        d.load_rows(2, rows)
    with pytest.raises(ValueError, match="set_from_wp: wp must be"):
        d.set_from_wp(torch.zeros(3, 10, 512))


def test_edit_styles_on_cpu_tensors():
    from dge_amd.infer import edit_styles, style_block_names
    assert tuple(style_block_names(14)) == S64_NAMES and len(style_block_names(26)) == 26          # 64^2 and 1024^2
    assert style_block_names(26)[16] == "layer16" and style_block_names(26)[17] == "output0"
    with pytest.raises(ValueError, match="not the StyleSpace code"):
        style_block_names(15)
    gen = torch.Generator().manual_seed(2)
    rows = [torch.randn(1, C, generator=gen) for C in S64_CHANNELS]
    sigma = [torch.rand(C, generator=gen) + 0.5 for C in S64_CHANNELS]
    out = edit_styles(rows, "layer6", 5, 2.0)
    assert out[6][0, 5] == rows[6][0, 5] + 2.0
    for g, (a, b) in enumerate(zip(out, rows)):
        assert a.data_ptr() != b.data_ptr()          # new rows
        keep = torch.ones_like(a, dtype=torch.bool)
        if g == 6:
            keep[0, 5] = False
        assert torch.equal(a[keep], b[keep])
    out = edit_styles(rows, "output3", 63, -3.0, sigma)          # - 3 sigma on a toRGB channel, by name
    assert out[12][0, 63] == rows[12][0, 63] + torch.tensor(-3.0 * float(sigma[12][63]))
    assert torch.equal(edit_styles(rows, 12, 63, -3.0, sigma)[12], out[12])          # by index
    for bad, msg in (((rows, "layer9", 0, 1.0), "no block"), ((rows, 14, 0, 1.0), "outside the 14 blocks"),
                     ((rows, "layer8", 32, 1.0), "outside the 32 channels"), ((rows, 0, 0, 1.0, sigma[:-1]), "one \\[C_g\\] tensor per block")):
        with pytest.raises(ValueError, match=msg):
            edit_styles(*bad)


def test_synthesis_refusals_that_need_no_gpu():
    syn = synthesis()
    with pytest.raises(ValueError, match="takes the place of wp"):
        syn(torch.zeros(1, 10, 512), styles=torch.zeros(sum(S64_CHANNELS)))
    with pytest.raises(ValueError, match="flat tensor"):
        syn(styles=torch.zeros(sum(S64_CHANNELS) + 1))
    with pytest.raises(ValueError, match="must be on the GPU"):
        syn(styles=torch.zeros(sum(S64_CHANNELS)))
    with pytest.raises(ValueError, match="style_grad_out needs"):
        syn(torch.zeros(1, 10, 512), style_grad_out=torch.zeros(4))
    with pytest.raises(ValueError, match="give wp"):
        syn()


def test_style_codes_is_a_lower_module():
    """tests/test_layering.py's rule for the new module: importing it never loads the training script, nor does it name it."""
    code = ("import sys, dge_amd\nimport dge_amd.style_codes\n"
            "assert 'dge_amd.e_align' not in sys.modules, sorted(m for m in sys.modules if m.startswith('dge_amd'))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    with open(os.path.join(ROOT, "deep-gan-encoders_amd", "style_codes.py")) as f:
        src = f.read()
    assert "from .e_align" not in src and "import e_align" not in src


def test_header_declares_the_new_symbols():
    from dge_amd._lib import SIGNATURES, S2GradEntry, S2SGradEntry
    import ctypes
    with open(os.path.join(ROOT, "include", "dge_hip.h")) as f:
        h = f.read()
    for name in ("dge_s2_style_grads_s", "dge_cols_mean_std", "dge_cols_mean_std_work_bytes"):
        assert f"int {name}(" in h and name in SIGNATURES, name
    assert "typedef struct dge_s2_sgrad_entry" in h
    # the by-value entry of the existing kernel did not grow, and the new one is no larger
    assert ctypes.sizeof(S2GradEntry) == 88 and ctypes.sizeof(S2SGradEntry) == 88
