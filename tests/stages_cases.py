"""Shared by tests/test_stages_host.py and tests/test_stages_gpu.py: an INDEPENDENT staged GAN step (it uses nothing of
``unet_bssfp_amd.gan`` and not ``oracle.gan_training_step``, which un-freezes the generator after the discriminator phase),
and tiny stand-in networks with the reference's module tables for the tests that are about files and plumbing."""
import torch
import torch.nn as nn
import torch.nn.functional as F

LOG_NAMES = ("gen_loss_adversarial", "gen_loss_recon_L1", "gen_loss_recon", "gen_loss", "discr_loss")


class StagedLoop:
    """The reference's training step (src/model.py:259-281) with a frozen set: ``frozen`` modules never train, AdamW (torch
    defaults) is built over the other parameters only, and the per-phase toggles RESTORE the flags (Lightning's
    ``toggle_optimizer`` / ``untoggle_optimizer``) instead of setting all of them.  ``head_grads`` keeps the generator-phase
    gradients of ``watch`` (name -> clone) of the latest step, taken before ``zero_grad``."""

    def __init__(self, gen, discr, frozen=(), lr=1e-3, recon_factor=1e2, watch=None):
        self.gen, self.discr, self.recon_factor = gen, discr, recon_factor
        self.frozen = {id(p) for m in frozen for p in m.parameters()}
        for net in (gen, discr):
            self._flags(net, True)
        self.g_opt = torch.optim.AdamW([p for p in gen.parameters() if id(p) not in self.frozen], lr=lr)
        self.d_opt = torch.optim.AdamW([p for p in discr.parameters() if id(p) not in self.frozen], lr=lr)
        self.watch = watch
        self.head_grads = {}

    def _flags(self, net, on):
        for p in net.parameters():
            p.requires_grad_(bool(on) and id(p) not in self.frozen)

    def step(self, x, y):
        bce = F.binary_cross_entropy_with_logits
        gen, discr = self.gen, self.discr
        self._flags(discr, False)
        y_hat = gen(x)
        logits = discr(x, y_hat)
        adv = bce(logits, torch.ones_like(logits))
        l1 = F.l1_loss(y_hat, y)
        recon = l1 * self.recon_factor                     # one reconstruction term: (L1) / 1 * recon_factor
        gen_loss = adv + recon
        gen_loss.backward()
        if self.watch is not None:
            self.head_grads = {n: p.grad.detach().clone() for n, p in self.watch.named_parameters() if p.grad is not None}
        self.g_opt.step()
        self.g_opt.zero_grad()
        self._flags(discr, True)
        self._flags(gen, False)
        y_fake = gen(x).detach()
        logits_fake, logits_real = discr(x, y_fake), discr(x, y)
        d_loss = (bce(logits_real, torch.ones_like(logits_real)) + bce(logits_fake, torch.zeros_like(logits_fake))) / 2
        d_loss.backward()
        self.d_opt.step()
        self.d_opt.zero_grad()
        self._flags(gen, True)
        return dict(gen_loss_adversarial=adv.detach(), gen_loss_recon_L1=l1.detach(), gen_loss_recon=recon.detach(),
                    gen_loss=gen_loss.detach(), discr_loss=d_loss.detach())


# ---- tiny networks with the reference's tables: gen.blocks[modality | 'unet'], discr.d1[modality] ------------------------------

class _TinyHead(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv3d(cin, cout, 1)
        self.bn = nn.BatchNorm3d(cout)

    def forward(self, x):
        return F.leaky_relu(self.bn(self.conv(x)), 0.2)


class TinyGenerator(nn.Module):
    def __init__(self, input_modality):
        super().__init__()
        self.input_modality = input_modality
        h6, h24 = _TinyHead(6, 4), _TinyHead(24, 4)
        unet = nn.Sequential(nn.Conv3d(4, 4, 3, padding=1), nn.LeakyReLU(0.1), nn.Conv3d(4, 6, 1))
        self.blocks = nn.ModuleDict({"dwi-tensor": h6, "pc-bssfp": h24, "bssfp": h24, "t1w": h6, "unet": unet})

    def forward(self, x):
        return self.blocks["unet"](self.blocks[self.input_modality](x))


class TinyDiscriminator(nn.Module):
    def __init__(self, modality):
        super().__init__()
        self.modality = modality
        d30, d12 = nn.Conv3d(30, 4, 2, 2), nn.Conv3d(12, 4, 2, 2)
        self.d1 = self.blocks = nn.ModuleDict({"dwi-tensor": d12, "pc-bssfp": d30, "bssfp": d30, "t1w": d12})
        self.final = nn.Conv3d(4, 1, 1)

    def forward(self, x, y):
        return self.final(F.leaky_relu(self.d1[self.modality](torch.cat([x, y], 1)), 0.2))


class TinyQueue:
    """``n`` patches of 8^3 per epoch for ``modality``, in the layout ``unpack_batch`` reads; seeded, the same every epoch"""

    def __init__(self, modality, n=4, seed=0):
        self.modality, self.n, self.seed = modality, n, seed
        self.patch_size = (8, 8, 8)

    def __len__(self):
        return self.n

    def batches(self, batch_size, **kw):
        g = torch.Generator().manual_seed(self.seed)
        cin = 24 if self.modality in ("bssfp", "pc-bssfp") else 6
        left = self.n
        while left > 0:
            b = min(batch_size, left)
            left -= b
            y = torch.rand(b, 6, 8, 8, 8, generator=g)
            x = y.clone() if self.modality == "dwi-tensor" else torch.rand(b, cin, 8, 8, 8, generator=g)
            batch = {"dwi-tensor_orig": {"data": y}, "dwi-tensor": {"data": y}}
            batch[self.modality] = {"data": x}             # ('dwi-tensor': the auto-encoder reads what it is to reproduce)
            yield batch
