"""What the noise-optimisation tests and tools/gen_golden_s2_noise.py share: the 64^2 StyleGAN2 model whose noise strengths are
away from 0 (the reference initialises them to 0, where the noise gradient vanishes), and a float64 restatement of the noise
regulariser of StyleGAN2's projector with its closed-form gradient and of the renormalisation."""
import torch

from tests.golden import recipe as R
from tests.helpers import s2_shapes

S2N_KW = dict(fmaps_base=2048, fmaps_max=128)
S2N_RES = (4, 8, 8, 16, 16, 32, 32, 64, 64)          # the conv layers' noise maps at 64^2, in layer order


def noise_strength(i):
    """Layer i's noise strength: magnitude about 0.1, alternating sign."""
    return 0.1 * (-1) ** i * (1 + 0.03 * i)


def s2n_state_dict():
    sd = R.fill_s2(s2_shapes(64, **S2N_KW), seed=11)
    for i in range(len(S2N_RES)):
        sd[f"synthesis.layer{i}.noise_strength"] = torch.tensor(noise_strength(i), dtype=torch.float32)
    return sd


def levels(R_):
    n = 1
    while (R_ >> (n - 1)) > 8:
        n += 1
    return n


def _left(x):          # roll(x, 1, w): element [y, x] is x[y, x - 1], wrapping
    return torch.cat((x[..., -1:], x[..., :-1]), dim=-1)


def _up(x):
    return torch.cat((x[..., -1:, :], x[..., :-1, :]), dim=-2)


def pyramid(n):
    """n [..., R, R] -> [n_0, n_1, ...]: 2x2 means down to the first level of side <= 8."""
    out = [n]
    while out[-1].shape[-1] > 8:
        x = out[-1]
        S = x.shape[-1] // 2
        x = x.reshape(*x.shape[:-2], S, 2, S, 2)
        out.append(x.mean(dim=(-3, -1)))
    return out


def reg_ref(n):
    """reg of maps n [..., R, R] (float64 in, float64 out [...]): sum over the levels of mean(n_l * roll_w)^2 + mean(n_l * roll_h)^2."""
    total = 0
    for x in pyramid(n.double()):
        total = total + (x * _left(x)).mean(dim=(-2, -1)) ** 2 + (x * _up(x)).mean(dim=(-2, -1)) ** 2
    return total


def reg_grad_ref(n):
    """The closed form of d reg / d n: at a fine pixel, sum over the levels of
    (2 / (N_l * 4^l)) * (m_w,l * (n_l[y, x-1] + n_l[y, x+1]) + m_h,l * (n_l[y-1, x] + n_l[y+1, x])) at the pooled pixel containing it."""
    n = n.double()
    g = torch.zeros_like(n)
    for l, x in enumerate(pyramid(n)):
        N = x.shape[-1] * x.shape[-2]
        mw = (x * _left(x)).mean(dim=(-2, -1), keepdim=True)
        mh = (x * _up(x)).mean(dim=(-2, -1), keepdim=True)
        right, down = torch.cat((x[..., 1:], x[..., :1]), dim=-1), torch.cat((x[..., 1:, :], x[..., :1, :]), dim=-2)
        t = (2.0 / (N * 4 ** l)) * (mw * (_left(x) + right) + mh * (_up(x) + down))
        g = g + t.repeat_interleave(2 ** l, dim=-2).repeat_interleave(2 ** l, dim=-1)
    return g


def normalize_ref(n):
    n = n.double()
    d = n - n.mean(dim=(-2, -1), keepdim=True)
    return d * torch.rsqrt((d * d).mean(dim=(-2, -1), keepdim=True))
