"""The modules below the training scripts do not depend on them: importing the losses, the StyleGAN2 generator, the collectives,
the generator adapters or the model builders never loads dge_amd.e_align."""
import os
import subprocess
import sys

from tests.conftest import ROOT

LOWER = ("losses", "stylegan2_generator", "s2_conv", "collectives", "generators", "models", "embed_step", "noise_maps")


def test_lower_modules_do_not_load_the_training_script():
    code = ("import sys, dge_amd\n"
            + "".join(f"import dge_amd.{m}\n" for m in LOWER)
            + "assert 'dge_amd.e_align' not in sys.modules, sorted(m for m in sys.modules if m.startswith('dge_amd'))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_lower_modules_do_not_name_the_training_script():
    for m in LOWER:
        with open(os.path.join(ROOT, "deep-gan-encoders_amd", m + ".py")) as f:
            src = f.read()
        assert "from .e_align" not in src and "import e_align" not in src, m
