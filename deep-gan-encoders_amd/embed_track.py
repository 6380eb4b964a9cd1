"""The best-loss / best-norm tracker of the inversion loops (embedding_v2, embedding_v2_biggan): the reference's `if` chains
(embedding_v2_styleGAN1.py:127-131, embedding_v2_styleGAN2.py:149-166, embedding_v2_BigGAN.py:168-177) run on the device
(dge_embed_track / dge_embed_track_rows), which keeps the latest best latent of each kind and a bounded ring of events
(iteration, kind, loss, norm); the host reads it once per image group and writes the reference's files from it."""
import os

import torch

from . import ops

EVENT_LOSS, EVENT_NORM = 0, 1


def tracker_rules(generator, iterations):
    """The reference's best-loss / best-norm `if` chains as parameters of dge_embed_track."""
    if generator == "sg1":        # armed at iterations//2 (min := that loss), hysteresis 1.05, no norm tracker, reset per group
        return dict(arm_rule=ops.TRACK_ARM_AT, arm_iter=iterations // 2, loss_hyst=1.05, norm_hyst=0.0, init=(0.0, 0.0),
                    reset_per_group=True)
    # iteration > 1000, hysteresis 1.03 / 1.05, minima start at 100 / 1000 and carry over between groups
    return dict(arm_rule=ops.TRACK_ARM_AFTER, arm_iter=1000, loss_hyst=1.03, norm_hyst=1.05, init=(100.0, 1000.0),
                reset_per_group=False)


class EmbedTracker:
    """The tracker's device state for one latent w [B, ...].  rows=False: one tracker for the whole w - istate [4] (iteration, events
    written, events dropped, armed), fstate [2] (minimal loss, minimal norm), events [cap,4], l2 [].  rows=True: a tracker per row of
    w, every state array with a leading B.  best_loss / best_norm have the shape of w in both forms.  `rules` is read at every
    update: the owner may change its entries."""

    def __init__(self, rules, events_cap=256, rows=False):
        self.rules, self.cap, self.rows = rules, int(events_cap), bool(rows)
        self.istate = self.fstate = self.best_loss = self.best_norm = self.events = self.l2 = None

    def reset(self, shape, device):
        """Start an image group on a latent of `shape`.  The tensors are allocated only when the shape or the device changes;
        otherwise the iteration counter and the event ring are zeroed in place (a captured iteration keeps reading these buffers).
        The minima start from rules["init"] after an allocation, with rules["reset_per_group"] and in the rows form; otherwise they
        carry over from the previous group (StyleGAN2: image k inherits image k-1's minima)."""
        shape, device = tuple(shape), torch.device(device)
        fresh = self.istate is None or tuple(self.best_loss.shape) != shape or self.istate.device != device
        if fresh:
            lead = shape[:1] if self.rows else ()

            def zeros(s, dtype=torch.float32):
                return torch.zeros(s, dtype=dtype, device=device)
            self.istate, self.fstate = zeros(lead + (4,), torch.int32), zeros(lead + (2,))
            self.events, self.l2 = zeros(lead + (self.cap, 4)), zeros(lead)
            self.best_loss, self.best_norm = zeros(shape), zeros(shape)
        else:
            self.istate.zero_()
            self.events.zero_()
        if fresh or self.rules["reset_per_group"] or self.rows:
            self.fstate.copy_(torch.tensor(self.rules["init"], dtype=torch.float32).expand_as(self.fstate))

    def update(self, loss, w):
        """One iteration: l2 = ||w|| (per row: ||w[b]||), then the tracker update on (loss, l2, w); two launches, no host sync."""
        r = self.rules
        l2, track = (ops.latent_l2_rows, ops.embed_track_rows) if self.rows else (ops.latent_l2, ops.embed_track)
        l2(w, out=self.l2)
        track(loss, self.l2, w, self.istate, self.fstate, self.best_loss, self.best_norm, self.events, r["arm_rule"], r["arm_iter"],
              r["loss_hyst"], r["norm_hyst"])

    def read(self):
        """The state on the host (one transfer): a dict, or in the rows form a list with one dict per row.  Events come oldest first;
        `dropped` counts those the ring has overwritten."""
        B, cap = self.istate.numel() // 4, self.cap
        # the three small state arrays travel as one float tensor (counters < 2^24 are exact in f32)
        host = torch.cat((self.istate.view(B, 4).float(), self.fstate.view(B, 2), self.events.view(B, cap * 4)), dim=1).cpu()
        out = []
        for b in range(B):
            it, cnt, dropped = (int(v) for v in host[b, :3])
            ev = host[b, 6:].view(cap, 4)
            idx = [k % cap for k in range(max(0, cnt - cap), cnt)]
            bl, bn = (self.best_loss[b:b + 1], self.best_norm[b:b + 1]) if self.rows else (self.best_loss, self.best_norm)
            out.append(dict(iteration=it, events=[(int(ev[i, 0]), int(ev[i, 1]), float(ev[i, 2]), float(ev[i, 3])) for i in idx],
                            dropped=dropped, min_loss=float(host[b, 4]), min_norm=float(host[b, 5]), best_loss=bl.clone(), best_norm=bn.clone()))
        return out if self.rows else out[0]


def write_tracker_files(tr, g, models_dir, result_dir):
    """The reference's outputs of the trackers for group g: the final best latent per kind (file names of
    embedding_v2_styleGAN2.py:156,163) and loss_min.txt lines (:159,166) from the event log."""
    last = {}
    loss_min = None
    with open(os.path.join(result_dir, "loss_min.txt"), "a+") as f:
        for it, kind, loss, norm in tr["events"]:
            if kind == EVENT_LOSS:
                loss_min = loss
                print("ep%d_iter%d_minImg%.5f_wNorm%f" % (g, it, loss, norm), file=f)
            else:
                print("ep%d_iter%d_Img%.5f_wNorm-min%f" % (g, it, loss, norm), file=f)
            last[kind] = (it, loss, norm, loss_min)
    if EVENT_LOSS in last:
        it, loss, norm, _ = last[EVENT_LOSS]
        torch.save(tr["best_loss"], os.path.join(models_dir, "id%d-iter%d-norm%f-imgLoss-min%f.pt" % (g, it, norm, loss)))
    if EVENT_NORM in last:
        it, loss, norm, lm = last[EVENT_NORM]
        torch.save(tr["best_norm"], os.path.join(models_dir, "id%d-iter%d-norm-min%f-imgLoss%f.pt" % (g, it, norm, lm if lm is not None else 0.0)))
