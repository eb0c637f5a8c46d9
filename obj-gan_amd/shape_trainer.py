"""Training driver of the shape generator (box layout -> per-box instance masks) on MI355X.

Same entry points as the reference (shape_generation/trainer.py:26-313): `condGANTrainer(output_dir, data_loader,
dataset)` with `build_models`, `define_optimizers`, `save_model`, `train`; the body of its loop (trainer.py:236-285) is
`train_step`, usable on its own.  What is built is the whole step -- generator, instance and global discriminator, the
perceptual term on the frozen VGG-19-bn (PCP_LAMBDA != 0: the network is loaded once from
<DATA_DIR>/pretrained/vgg19_bn-c79401a0.pth, a missing file is refused before any work), gradient clipping, Adam, the
EMA copy, the checkpoints, `Score/scores_N.txt`, the DISPLAY_INTERVAL grids `Image/{G,D,G2,D2}_average_<iter>.png`
(`save_img_results`, trainer.py:149-206) and `sampling` (trainer.py:316-401), the dump of one mask PNG per test image.
NOT built: data-parallel training over several GPUs.

Results-preserving differences:
  * parameters, gradients and Adam moments of each network live in flat arenas (`trainer.ParamArena`): one Adam launch
    per network, one EMA launch;
  * `clip_grad_norm_(RNN_GRAD_CLIP)` is `ops.box_train_clip` + the gated Adam: the norm never reaches the host;
  * the one-hot box maps are written on the device from the compact batch (`shapeDataset.prepare_data`), their maximum
    over the boxes is taken once per step;
  * discriminator weights are frozen during the generator step (the reference zeroes those gradients before use);
  * nothing is read back from the device unless the step prints or a checkpoint is written; pcp_score accumulates on
    the device and is read once per epoch (it is never reset between epochs, as in the reference);
  * the grids and the mask dump are composed on the device (`miscc.shape_utils`, `ops.mask_to_rgb8`): only finished
    uint8 arrays leave it.  Defined where the reference is not: a constant panel or mask (its 0 / 0) is 0, an image
    without a box is skipped by `sampling` and counted, and a grid shows min(8, batch size) images;
  * the images, which only the grids show, are read from `<split>_imgs.bigfile` when a grid is drawn; a data directory
    without that file trains without grids, after one notice.
Kept as it is: the three optimizers are re-created at every epoch (trainer.py:226), so their moments and step counts
start from zero each epoch; lr_rate *= 0.98 for epochs above 50.
"""
import ntpath
import os
import time

import numpy as np
import torch

from miscc.config import cfg
from miscc.utils import mkdir_p, weights_init
from miscc.shape_losses import ins_discriminator_loss, glb_discriminator_loss, generator_loss, check_pcp_lambda
from model import SHP_G_NET, INS_D_NET, GLB_D_NET, vgg19_bn, vgg_weights_path
from trainer import ParamArena, ArenaAdam
from objgan_hip import ops
import shapeDataset

EMA_DECAY = 0.999
# zlib level of the PNG files (Pillow's default is 6).  The pixels are the contract, not the file bytes: a grid of 2.8 MB
# takes 65 ms to encode at level 6 and 46 ms at level 1 for files of the same size within 2 % (LAB.md section 23).
PNG_COMPRESS_LEVEL = 1


class ClippedArenaAdam(object):
    """clip_grad_norm_(max_norm) + torch.optim.Adam on a ParamArena with the clip coefficient and the step count on the
    device: created fresh (zero moments, step 0) like the optimizer it stands for."""

    def __init__(self, arena, lr, max_norm, betas=(0.5, 0.999), eps=1e-8):
        self.arena, self.lr, self.max_norm, self.betas, self.eps = arena, float(lr), float(max_norm), betas, eps
        dev = arena.flat.device
        arena.exp_avg.zero_()
        arena.exp_avg_sq.zero_()
        self.state = torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64, device=dev)
        self.clip = torch.ones(2, dtype=torch.float32, device=dev)        # divisor, gradient norm
        self.coef = torch.zeros(3, dtype=torch.float32, device=dev)
        self.partials = torch.zeros(256, dtype=torch.float64, device=dev)

    def zero_grad(self):
        self.arena.zero_grad()

    def step(self):
        a = self.arena
        if hasattr(ops, "wgrad_join"):
            ops.wgrad_join()
        a.sync_grads()
        a.epoch[0] += 1
        ops.box_train_clip(a.grad[:a.n], self.max_norm, self.partials, self.clip)
        ops.adam_step_gated_(a.flat, a.grad, a.exp_avg, a.exp_avg_sq, self.lr, self.betas[0], self.betas[1], self.eps,
                             self.state, self.clip, self.coef, grad_scale=-1.0, n=a.n)
        ops.repack_arena(a.epoch)


def _fresh_adam(arena, lr):
    """a new torch.optim.Adam in the reference: zero moments, step 0"""
    arena.exp_avg.zero_()
    arena.exp_avg_sq.zero_()
    arena.step_count = 0
    arena.gate_state = None
    return ArenaAdam(arena, lr, betas=(0.5, 0.999))


def path_leaf(path):
    head, tail = ntpath.split(path)
    return tail or ntpath.basename(head)


class condGANTrainer(object):
    def __init__(self, output_dir, data_loader, dataset, device=None):
        self.model_dir = os.path.join(output_dir, 'Model')
        self.image_dir = os.path.join(output_dir, 'Image')
        self.score_dir = os.path.join(output_dir, 'Score')
        if cfg.TRAIN.FLAG:
            mkdir_p(self.model_dir)
            mkdir_p(self.image_dir)
            mkdir_p(self.score_dir)
        self.device = torch.device(device if device is not None else ("cuda:0" if cfg.CUDA else "cpu"))
        self.batch_size = cfg.TRAIN.BATCH_SIZE
        self.max_epoch = cfg.TRAIN.MAX_EPOCH
        self.snapshot_interval = cfg.TRAIN.SNAPSHOT_INTERVAL
        self.print_interval = cfg.TRAIN.PRINT_INTERVAL
        self.display_interval = int(cfg.TRAIN.DISPLAY_INTERVAL)
        self.dataset = dataset
        self.ixtoword = getattr(dataset, 'ixtoword', None)
        self.cats_dict = dataset.cats_dict
        self.cats_index_dict = dataset.cats_index_dict
        self.num_classes = len(self.cats_index_dict)
        self.data_loader = data_loader
        self.num_batches = len(data_loader) if data_loader is not None else 0
        self.clip_norm = float(cfg.TRAIN.get("RNN_GRAD_CLIP", 0.25))
        self.netG = None
        self.vgg = None
        self._png_pool, self._png_jobs = None, []

    # ---- networks ----
    def build_models(self):
        netG, netINSD, netGLBD = SHP_G_NET(self.num_classes), INS_D_NET(self.num_classes), GLB_D_NET(self.num_classes)
        for net in (netG, netINSD, netGLBD):
            net.apply(weights_init)
        epoch = 0
        if cfg.TRAIN.NET_G != '':
            netG.load_state_dict(torch.load(cfg.TRAIN.NET_G, map_location="cpu"))
            print('Load G from: ', cfg.TRAIN.NET_G)
            name = path_leaf(cfg.TRAIN.NET_G)
            epoch = int(name[name.rfind('_') + 1:name.rfind('.')]) + 1
            folder = os.path.dirname(cfg.TRAIN.NET_G)
            for net, leaf in ((netINSD, 'netINSD.pth'), (netGLBD, 'netGLBD.pth')):
                print('Load %s from: ' % leaf[3:-4], os.path.join(folder, leaf))
                net.load_state_dict(torch.load(os.path.join(folder, leaf), map_location="cpu"))
        vgg = None
        if float(cfg.TRAIN.SMOOTH.get("PCP_LAMBDA", 0.0)) != 0.0:
            check_pcp_lambda(cfg.TRAIN.SMOOTH.PCP_LAMBDA, vgg_weights_path())
            vgg = vgg19_bn(pretrained=True)
            print('Load the perceptual network from: ', vgg_weights_path())
        self.attach(netG, netINSD, netGLBD, vgg)
        return [netG, netINSD, netGLBD, epoch]

    def attach(self, netG, netINSD, netGLBD, vgg=None):
        """move the networks to the device and re-home their parameters into flat arenas; vgg: the frozen perceptual
        network (model.VGG), needed exactly when PCP_LAMBDA != 0"""
        self.vgg = vgg.to(self.device) if vgg is not None else None
        self.pcp_score = torch.zeros((), dtype=torch.float32, device=self.device)
        self.netG, self.netINSD, self.netGLBD = (n.to(self.device).train() for n in (netG, netINSD, netGLBD))
        self.arenaG, self.arenaINSD, self.arenaGLBD = (ParamArena(n) for n in (self.netG, self.netINSD, self.netGLBD))
        self.avg_param_G = self.arenaG.flat.clone()
        self.noise = torch.empty(self.batch_size, cfg.ROI.BOXES_NUM, self.num_classes * 4, device=self.device)

    def define_optimizers(self, lr_rate):
        self.optimizerG = ClippedArenaAdam(self.arenaG, cfg.TRAIN.GENERATOR_LR * lr_rate, self.clip_norm)
        self.optimizerINSD = _fresh_adam(self.arenaINSD, cfg.TRAIN.DISCRIMINATOR_LR * lr_rate)
        self.optimizerGLBD = _fresh_adam(self.arenaGLBD, cfg.TRAIN.DISCRIMINATOR_LR * lr_rate)
        return self.optimizerG, self.optimizerINSD, self.optimizerGLBD

    # ---- one iteration (reference trainer.py:236-285) ----
    def train_step(self, batch, noise=None):
        """batch: shapeDataset.prepare_data's dict -> the losses and the generator's gradient norm as device scalars
        (gpcp_loss and this step's pcp_score are zeros when the perceptual term is off)"""
        R = batch["max_num_roi"]
        fwd = batch["bbox_maps_fwd"]
        if noise is None:
            self.noise.normal_(0, 1)
            noise = self.noise[:, :R]
        fake_hmaps = self.netG(noise, fwd, batch["bbox_maps_bwd"], batch["bbox_fmaps"])
        pooled_maps = ops.box_max(fwd)

        self.optimizerINSD.zero_grad()
        with ops.direct_wgrad_scope():
            errINSD = ins_discriminator_loss(self.netINSD, batch["hmaps"], fake_hmaps, fwd)
            errINSD.backward()
        self.optimizerINSD.step()

        self.optimizerGLBD.zero_grad()
        with ops.direct_wgrad_scope():
            errGLBD = glb_discriminator_loss(self.netGLBD, batch["pooled_hmaps"], fake_hmaps, fwd, pooled_maps)
            errGLBD.backward()
        self.optimizerGLBD.step()

        self.optimizerG.zero_grad()
        self.arenaINSD.set_requires_grad(False)
        self.arenaGLBD.set_requires_grad(False)
        try:
            with ops.direct_wgrad_scope():
                res = generator_loss(self.netINSD, self.netGLBD, self.vgg, batch["hmaps"], fake_hmaps, fwd, pooled_maps)
                errG, logs = res[0], res[1]
                insg, glbg = logs[0], logs[1]
                errG.backward()
        finally:
            self.arenaINSD.set_requires_grad(True)
            self.arenaGLBD.set_requires_grad(True)
        self.optimizerG.step()
        ops.ema_update_(self.avg_param_G, self.arenaG.flat, EMA_DECAY)
        if self.vgg is not None:
            gpcp, score = logs[2].detach(), res[2]
            self.pcp_score += score                      # on the device: read once per epoch
        else:
            gpcp = score = torch.zeros_like(self.pcp_score)
        return {"errINSD": errINSD.detach(), "errGLBD": errGLBD.detach(), "errG": errG.detach(),
                "insg_loss": insg.detach(), "glbg_loss": glbg.detach(), "gpcp_loss": gpcp, "pcp_score": score,
                "fake_hmaps": fake_hmaps.detach(), "clip": self.optimizerG.clip}

    # ---- checkpoints ----
    def save_model(self, epoch):
        """Model/netG_epoch_N.pth with the EMA weights, netINSD.pth / netGLBD.pth with the live ones"""
        a = self.arenaG
        backup = a.flat.clone()
        a.flat.copy_(self.avg_param_G)
        try:
            torch.save({k: v.detach().cpu().clone() for k, v in self.netG.state_dict().items()},
                       '%s/netG_epoch_%d.pth' % (self.model_dir, epoch))
        finally:
            a.flat.copy_(backup)
        for net, leaf in ((self.netINSD, 'netINSD.pth'), (self.netGLBD, 'netGLBD.pth')):
            torch.save({k: v.detach().cpu().clone() for k, v in net.state_dict().items()},
                       '%s/%s' % (self.model_dir, leaf))

    # ---- snapshot grids (reference trainer.py:149-206) ----
    @torch.no_grad()
    def save_img_results(self, batch, noise, gen_iterations, name='current', imgs=None, wait=True):
        """Image/{G,D,G2,D2}_<name>_<n>.png: the generated (G) and the real (D) masks of the first min(8, B) images of
        `batch` beside their images, every panel normalised by its own range (G_, D_) and raw (G2_, D2_).  The generator
        runs with the EMA weights swapped in through the arena; the live weights, the moments and the noise stream are
        as before afterwards.  imgs: [>= nvis, 3, S, S] in [-1, 1] (None: read from the data set by the batch's keys).
        Only the four finished uint8 grids leave the device.  The PNG files are encoded by worker threads (the encoder
        leaves the interpreter free): wait=False returns once the grids are on the host and leaves the files to
        `finish_images`, which the next call and the end of `train` run.  -> the paths written."""
        from PIL import Image
        from miscc.shape_utils import build_super_images, build_super_images2, caption_strip
        font_max, font_size, mw = 20, 12, int(cfg.ROI.BOXES_NUM)
        nvis = min(8, int(noise.size(0)))
        a = self.arenaG
        backup = a.flat.clone()
        a.flat.copy_(self.avg_param_G)
        a.epoch[0] += 1                                   # (the packed filter banks are keyed on it)
        try:
            # only the images that are shown: the generator couples nothing across the images of a batch
            fake_hmaps = self.netG(noise[:nvis], batch["bbox_maps_fwd"][:nvis], batch["bbox_maps_bwd"][:nvis],
                                   batch["bbox_fmaps"][:nvis])
        finally:
            a.flat.copy_(backup)
            a.epoch[0] += 1
            ops.repack_arena(a.epoch)
        S = int(fake_hmaps.size(-1))
        if imgs is None:
            imgs = self.dataset.images_for(batch["keys"][:nvis])
        imgs = imgs[:nvis].to(self.device, torch.float32)
        captions = np.zeros((nvis, mw), np.int64)
        rois, num_rois = np.asarray(batch["rois"]), np.asarray(batch["num_rois"]).reshape(-1)
        for b in range(nvis):
            for r in range(min(int(num_rois[b]), mw)):
                captions[b, r] = self.cats_dict[int(rois[b, r, 4])][0]
        strip = caption_strip(captions, self.ixtoword, nvis, S, font_max, font_size, mw, self.device)
        self.finish_images()
        if self._png_pool is None:
            from concurrent.futures import ThreadPoolExecutor
            self._png_pool = ThreadPoolExecutor(max_workers=4)
        paths = []
        for tag, fn, maps in (("G", build_super_images, fake_hmaps), ("D", build_super_images, batch["hmaps"]),
                              ("G2", build_super_images2, fake_hmaps), ("D2", build_super_images2, batch["hmaps"])):
            grid, _ = fn(imgs, captions, self.ixtoword, maps[:nvis], S, lr_imgs=None, font_max=font_max,
                         font_size=font_size, max_word_num=mw, strip=strip)
            paths.append('%s/%s_%s_%d.png' % (self.image_dir, tag, name, gen_iterations))
            self._png_jobs.append(self._png_pool.submit(Image.fromarray(grid).save, paths[-1],
                                                        compress_level=PNG_COMPRESS_LEVEL))
        if wait:
            self.finish_images()
        return paths

    def finish_images(self):
        """wait for the PNG files of earlier display calls; an error of a writer is raised here"""
        jobs, self._png_jobs = self._png_jobs, []
        for job in jobs:
            job.result()

    def display_ready(self):
        """whether train() can draw the grids: an interval above 0 and a data set that has its images; says once why not"""
        if self.display_interval <= 0:
            return False
        has = getattr(self.dataset, 'has_images', None)
        if has is not None and has():
            return True
        print('No %s: this run trains without the DISPLAY_INTERVAL grids (they show the images).'
              % (self.dataset.imgs_path() if has is not None else 'image file in this data set'))
        return False

    # ---- one mask PNG per image (reference trainer.py:316-401) ----
    @torch.no_grad()
    def sampling(self, split_dir, noise=None, all_boxes=False):
        """Load cfg.TRAIN.NET_G and write <NET_G without .pth>/<split>/single/<key>_<word>.png for every image of the
        loader's whole batches: the mask of its first box, (v - min) / (max - min) * 255 on three channels, <word> the
        first word of the box's category.  all_boxes (an extension): every box r, as <key>_<r>_<word>.png.  Per batch one
        generator forward, one `ops.mask_to_rgb8` launch, one device-to-host copy.  An image without a box (the
        reference: IndexError) is skipped; the count is printed.  noise: [B, BOXES_NUM, 4 * classes] used for every
        batch, or a sequence of such tensors, one per batch (None: drawn per batch).  -> (files written, images skipped)"""
        from PIL import Image
        if cfg.TRAIN.NET_G == '':
            print('Error: the path for models is not found!')
            return 0, 0
        if split_dir == 'test':
            split_dir = 'valid'
        netG = SHP_G_NET(self.num_classes)
        netG.load_state_dict(torch.load(cfg.TRAIN.NET_G, map_location="cpu"))
        netG = netG.to(self.device).eval()
        print('Load G from: ', cfg.TRAIN.NET_G)
        model_dir = cfg.TRAIN.NET_G
        save_dir = '%s/%s' % (model_dir[:model_dir.rfind('.pth')], split_dir)
        mkdir_p(save_dir)
        z = torch.empty(self.batch_size, cfg.ROI.BOXES_NUM, self.num_classes * 4, device=self.device)
        written = skipped = 0
        for step, data in enumerate(self.data_loader):
            if step % 100 == 0:
                print('step: ', step)
            num = [int(n) for n in data[7]]
            skipped += sum(1 for n in num if n < 1)
            if max(num) < 1:
                continue
            batch = shapeDataset.prepare_data(data, self.device, self.num_classes)
            R = batch["max_num_roi"]
            if noise is None:
                z.normal_(0, 1)
                zz = z
            else:
                zz = (noise if torch.is_tensor(noise) else noise[step]).to(self.device)
            fake_hmaps = netG(zz[:, :R], batch["bbox_maps_fwd"], batch["bbox_maps_bwd"], batch["bbox_fmaps"])
            todo = [(b, r) for b, n in enumerate(num) for r in range(n if all_boxes else min(n, 1))]
            rgb = ops.mask_to_rgb8(fake_hmaps, [b * R + r for b, r in todo]).cpu().numpy()
            for im, (b, r) in zip(rgb, todo):
                stem = '%s/single/%s' % (save_dir, batch["keys"][b])
                folder = stem[:stem.rfind('/')]
                if not os.path.isdir(folder):
                    print('Make a new folder: ', folder)
                    mkdir_p(folder)
                word = self.ixtoword[self.cats_dict[int(batch["rois"][b, r, 4])][0]].encode('ascii', 'ignore').decode('ascii')
                Image.fromarray(im).save(('%s_%d_%s.png' % (stem, r, word)) if all_boxes else '%s_%s.png' % (stem, word),
                                         compress_level=PNG_COMPRESS_LEVEL)
                written += 1
        print('sampling: %d files in %s/single, %d images without a box skipped' % (written, save_dir, skipped))
        return written, skipped

    def write_score(self, epoch):
        """the epoch's one host read of the accumulated perceptual score (reference trainer.py:304-308; never reset)"""
        pcp_score = float(self.pcp_score)
        print('pcp_score: ', pcp_score)
        with open('%s/scores_%d.txt' % (self.score_dir, epoch), 'w') as f:
            f.write('pcp_score %f' % pcp_score)
        return pcp_score

    # ---- the loop ----
    def train(self):
        start_epoch = self.build_models()[3]
        gap = "Not built here: data-parallel training over several GPUs (--gpu '0,1' uses the first device)."
        if self.vgg is None:
            print(gap + '  PCP_LAMBDA = 0: this run leaves the perceptual term out (gpcp_loss and pcp_score stay 0).')
        else:
            print(gap)
        display = self.display_ready()
        fixed_noise = torch.empty_like(self.noise)
        if display:
            # drawn once, from a generator of its own: the training noise is the same stream with and without grids
            gen = torch.Generator(device=self.device)
            gen.manual_seed(torch.initial_seed())
            fixed_noise.normal_(0, 1, generator=gen)
        gen_iterations = 0
        lr_rate = 1
        for epoch in range(start_epoch, self.max_epoch):
            start_t = time.time()
            if epoch > 50 and lr_rate > cfg.TRAIN.GENERATOR_LR / 10.:
                lr_rate *= 0.98
            self.define_optimizers(lr_rate)
            for step, data in enumerate(self.data_loader, 1):
                batch = shapeDataset.prepare_data(data, self.device, self.num_classes)
                out = self.train_step(batch)
                gen_iterations += 1
                if display and gen_iterations % self.display_interval == 0:
                    self.save_img_results(batch, fixed_noise[:, :batch["max_num_roi"]], gen_iterations, name='average',
                                          wait=False)
                if gen_iterations % self.print_interval == 0:
                    vals = {k: float(out[k]) for k in ("errINSD", "errGLBD", "insg_loss", "glbg_loss", "gpcp_loss")}
                    elapsed = time.time() - start_t
                    print('| epoch {:3d} | {:5d}/{:5d} batches | ms/batch {:5.2f} | '
                          .format(epoch, step, self.num_batches, elapsed * 1000. / self.print_interval))
                    # (the reference's G_logs; without the term -- PCP_LAMBDA = 0 -- the line keeps its two entries)
                    pcp = 'gpcp_loss: %.2f ' % vals["gpcp_loss"] if self.vgg is not None else ''
                    print('errINSD: %.2f \nerrGLBD: %.2f \ninsg_loss: %.2f glbg_loss: %.2f %s'
                          % (vals["errINSD"], vals["errGLBD"], vals["insg_loss"], vals["glbg_loss"], pcp))
                    start_t = time.time()
            self.write_score(epoch)
            if epoch % self.snapshot_interval == 0:
                self.save_model(epoch)
        self.save_model(self.max_epoch)
        self.finish_images()
