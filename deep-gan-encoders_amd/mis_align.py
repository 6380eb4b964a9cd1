"""The `E_mis_align_cropping_s1.py` iteration on the HIP path (reference :109-206).

What the shipped loop does, and what is kept: G -> E -> G as in E_align_s2; Grad-CAM++ masks of both image batches,
guided-back-propagation gradients, JET overlays (metric/grad_cam.py); four *logged* image-space `space_loss`
evaluations (gradients, images, masks, overlays).  Every one of them is built from detached tensors (:175-191), so
`loss_tsa.backward()` reaches only LPIPS's own `lin` weights and the first `E_optimizer.step()` finds no gradient:
the encoder is trained by the latent phase (`0.01 * loss_w`, :199-205) alone.  The second synthesis therefore runs
without a gradient tape here.  `loss_c` (:197, logged only) is not produced.
"""
import torch

from . import losses, ops
from .e_align import EAlignStep
from .grad_cam import GradCamPlusPlus, GuidedBackPropagation, mask2cam
from .train_step import TrainStep


class MisAlignStep(EAlignStep):
    def __init__(self, generator, E, lpips_model, vgg16, fused_attention=True, **kw):
        """`vgg16`: dge_amd.grad_cam.VGG16 (torchvision vgg16 layout), shared by Grad-CAM++ and guided back-propagation
        as in E_mis_align_cropping_s1.py:99-106."""
        super().__init__(generator, E, lpips_model, **kw)
        self.grad_cam_plus_plus = GradCamPlusPlus(vgg16, vgg16.final_layer)
        self.gbp = GuidedBackPropagation(vgg16)
        self.fused_attention = fused_attention

    _first_pass = TrainStep._first_pass          # the plain head: no prefetched pass, no early weight re-pack

    def step(self, iteration, z=None, noises=None, gen_noises=(None, None), new_z=None):
        z, imgs1, w1, const2, w2, imgs2 = self._head(iteration, z, noises, gen_noises, new_z, synth_grad=False)
        with torch.no_grad():
            # attention maps (:159-170)
            if self.fused_attention:       # one forward + one backward per batch instead of two of each (same results)
                mask_1, grad_1 = self.grad_cam_plus_plus.with_input_gradient(imgs1)
                mask_2, grad_2 = self.grad_cam_plus_plus.with_input_gradient(imgs2)
            else:
                mask_1 = self.grad_cam_plus_plus(imgs1, None)
                mask_2 = self.grad_cam_plus_plus(imgs2, None)
                grad_1 = self.gbp(imgs1)
                grad_2 = self.gbp(imgs2)
            heat_1, cam_1 = mask2cam(mask_1, imgs1)
            heat_2, cam_2 = mask2cam(mask_2, imgs2)
            gctx = losses.GlobalBatch(self.world) if (self.dist_on and self.exact_ddp) else None
            # logged image-space terms (:172-191); values only
            _, info_grad = losses.space_loss(grad_1, grad_2, lpips_model=self.lpips, global_batch=gctx)
            l_imgs, info_imgs = losses.space_loss(imgs1, imgs2, lpips_model=self.lpips, global_batch=gctx)
            l_mask, info_mask = losses.space_loss(mask_1, mask_2, lpips_model=self.lpips, global_batch=gctx)
            l_cam, info_cam = losses.space_loss(cam_1, cam_2, lpips_model=self.lpips, global_batch=gctx)
            loss_tsa = l_imgs + l_mask + l_cam
        # latent phase (:199-205)
        loss_w, info_w = losses.space_loss(w1, w2, image_space=False, global_batch=gctx)
        loss_mtv = loss_w * 0.01
        self.opt.zero_grad()
        loss_mtv.backward()
        gs = self._sync_grads()
        self.opt.step(grad_scale=gs)
        ops.zero_arena_end()
        self.last = dict(imgs1=imgs1, imgs2=imgs2, w1=w1, w2=w2.detach(), const2=const2, mask_1=mask_1, mask_2=mask_2,
                         grad_1=grad_1, grad_2=grad_2, heatmap_1=heat_1, heatmap_2=heat_2, cam_1=cam_1, cam_2=cam_2,
                         loss_tsa=loss_tsa, info_imgs=info_imgs, info_mask=info_mask, info_Gcam=info_cam, info_grad=info_grad,
                         loss_w=loss_w.detach(), info_w=info_w)
        return self.last
