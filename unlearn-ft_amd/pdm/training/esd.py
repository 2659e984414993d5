"""ESD on the MI355X engine (the reference's baselines/erasing/esd_diffusers.py): fine-tune some modules of the pruned student
so that its prediction for `erase_from` moves away from the concept, e_f - ng (e_p - e_n), with the three predictions taken from
the frozen original weights at a partially sampled latent.

Per iteration (esd_diffusers.py:59-108): the three host draws (pdm/utils/esd.py draws), `iteration` DDIM steps of the 50-step
schedule with the fine-tuned weights at guidance 3 (the captured DDIM loop, which reads the weight arenas in place), the frozen
predictions as ONE batch of 3 rows (2 when concept == erase_from), the student's prediction with a tape, pdmk_esd_head, the
hand-written backward and torch.optim.Adam on the trainable subset (pdmk_adamw_segments, weight decay 0).

The backward still forms the weight gradients of frozen layers; nothing reads them and nothing zeroes them.
"""
import torch

from .. import _pdmk as k
from ..models.unet.spec import padc
from ..utils import esd as E
from .bilevel import FusedAdamW


class EsdTrainer:
    def __init__(self, frozen, student, pipe, train_method, lr=1e-5, negative_guidance=1.0, nsteps=E.NSTEPS,
                 guidance=E.GUIDANCE, graph=True):
        """frozen / student: the same checkpoint loaded twice (train=False / train=True); pipe: a DDIM pipeline over `student`."""
        if not student.store.train or frozen.dtype != student.dtype:
            raise ValueError("EsdTrainer: the student needs train=True and the frozen model's dtype")
        self.frozen, self.student, self.pipe = frozen, student, pipe
        self.dev, self.dtype = student.device, student.dtype
        self.ng, self.nsteps, self.guidance, self.graph = float(negative_guidance), int(nsteps), float(guidance), bool(graph)
        store = student.store
        self.entries = E.trainable_entries(store.entries, train_method)
        self.names = [n for n in store.state_dict_names() if n in {s[0] for e in self.entries for s in e.srcs}]
        self.segments = E.segments(self.entries)
        store.defer_wt = False              # the optimiser step refreshes the dgrad copies itself
        self.opt = FusedAdamW(store, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, segments=self.segments)
        sch = pipe.scheduler
        self.t_of = {i: E.prediction_timestep(sch, i, self.nsteps) for i in range(1, max(self.nsteps - 1, 2))}
        self._emb = {}

    # ---- text
    def embed(self, text):
        """[1, T, ctx] embedding of one text, encoded once (the encoder is frozen)."""
        if text not in self._emb:
            with torch.no_grad():
                self._emb[text] = self.pipe.text_encoder(self.pipe._tokenize([text]))[0]
        return self._emb[text]

    def _ehs2d(self, embs):
        e = torch.cat([x.to(self.dev) for x in embs], 0)
        return e.to(self.dtype).reshape(e.shape[0] * e.shape[1], e.shape[2]).contiguous()

    # ---- the deterministic part of an iteration
    @torch.no_grad()
    def frozen_predictions(self, x, t, emb_p, emb_n, emb_f, same):
        """The original weights' predictions at (x, t) as ONE batch: rows concept, '' and - unless `same` - erase_from.  Returns
        (the U-Net input rows, the timesteps, the prediction rows [R * HW, ld])."""
        B, C, H, W = x.shape
        if B != 1:
            raise ValueError("EsdTrainer: batch 1")
        HW, cp, R = H * W, padc(C), 2 if same else 3
        x = x.to(self.dev, torch.float32)
        xin = torch.empty((R * HW, cp), device=self.dev, dtype=self.dtype)
        k.nchw_to_nhwc(x.expand(R, C, H, W).contiguous(), xin, R, C, HW, cp)
        tt = torch.full((R,), int(t), device=self.dev, dtype=torch.int64)
        ehs = self._ehs2d([emb_p, emb_n] if same else [emb_p, emb_n, emb_f])
        pf, _ = self.frozen.forward_nhwc(xin, tt, ehs, R, H, W, train=False)
        return xin, tt, pf.t

    @torch.no_grad()
    def student_pass(self, xin, tt, pf, emb_f, same, C, H, W):
        """The student's prediction for erase_from with a tape, pdmk_esd_head and the backward; returns the loss [1]."""
        HW = H * W
        e_p, e_n = pf[:HW], pf[HW:2 * HW]
        e_f = e_n if same else pf[2 * HW:]
        pred, _ = self.student.forward_nhwc(xin[:HW], tt[:1], self._ehs2d([emb_f]), 1, H, W, train=True)
        loss = k.zeros((1,), self.dev, torch.float64)
        n = C * HW
        pred.g = torch.empty_like(pred.t)           # every column is written by the head (padding: zeros)
        k.esd_head(pred.t, e_p, e_n, e_f, self.ng, loss, 0, pred.g, HW, C, pred.t.stride(0), pf.stride(0), pred.g.stride(0),
                   1.0 / n, 2.0 / n)
        self.student.engine.grad_ready_cb = None
        self.student.engine.backward()
        return loss

    def loss_and_grads(self, x, t, emb_p, emb_n, emb_f, same):
        """x: fp32 [1, C, H, W] latents; t: the U-Net timestep; emb_*: [1, T, ctx] embeddings of the concept, '' and erase_from;
        same: concept == erase_from (e_f := e_n).  Frozen and student forward, head, backward: the gradients are added to the
        student's gradient arena; returns the loss as a float64 device tensor [1]."""
        xin, tt, pf = self.frozen_predictions(x, t, emb_p, emb_n, emb_f, same)
        return self.student_pass(xin, tt, pf, emb_f, same, *x.shape[1:])

    def step(self, x, t, emb_p, emb_n, emb_f, same):
        """loss_and_grads and one Adam step on the trainable subset (which clears its gradients and refreshes the compute
        copies); returns the loss, still on the device."""
        loss = self.loss_and_grads(x, t, emb_p, emb_n, emb_f, same)
        self.opt.step(grad_scale=1.0, zero_grad=True)
        return loss

    # ---- one iteration of the reference's loop
    def sample(self, emb_p, emb_n, latents, iteration):
        """`iteration` DDIM steps with the fine-tuned weights (esd_diffusers.py:76-84)."""
        return self.pipe.generate_samples(prompt_embeds=emb_p, negative_prompt_embeds=emb_n, latents=latents,
                                          num_inference_steps=self.nsteps, guidance_scale=self.guidance, output_type="latent",
                                          end_iteration=iteration, graph=self.graph).images

    def iteration(self, pairs, draw):
        """draw: (pair index, iteration, initial latents) of pdm.utils.esd.draws."""
        index, it, latents = draw
        concept, erase_from = pairs[index]
        emb_p, emb_n, emb_f = self.embed(concept), self.embed(""), self.embed(erase_from)
        x = self.sample(emb_p, emb_n, latents, it)
        return self.step(x, self.t_of[it], emb_p, emb_n, emb_f, concept == erase_from)

    def trained_state_dict(self):
        """{name: fp32 CPU tensor} of the trainable tensors, reference shapes."""
        sd = self.student.state_dict()
        return {n: sd[n] for n in self.names}


def train(args, log=print):
    """The script's body: returns (checkpoint path, trainer)."""
    import numpy as np
    from ..utils.load_models import FrozenModels, cuda_device, inference_config
    E.check_train_method(args.train_method)                 # before anything is loaded
    pairs = E.build_pairs(args.erase_concept, args.erase_from)
    path = E.checkpoint_path(args.save_path, args.erase_concept, args.erase_from, args.train_method, args.negative_guidance,
                             args.iterations)
    if args.ckpt_path is None:
        raise ValueError("--ckpt_path is required (the pruned checkpoint directory: arch_vector.pt + unet/)")
    log(pairs)
    config = inference_config(args.base_config_path, args.model_id, args.tiny, mixed_precision=args.mixed_precision)
    device = str(args.device)
    models = FrozenModels(config, cuda_device(device.split(":")[1] if ":" in device else 0))
    frozen = models.load_unet(args.ckpt_path)
    student = models.load_unet(args.ckpt_path, train=True)
    pipe = models.pipeline(student, kind="ddim")
    tr = EsdTrainer(frozen, student, pipe, args.train_method, lr=args.lr, negative_guidance=args.negative_guidance,
                    graph=bool(args.graph))
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    side = args.image_size // 8
    draws = E.draws(len(pairs), tr.nsteps, (1, student.cfg.in_channels, side, side))
    for i in range(args.iterations):
        loss = tr.iteration(pairs, next(draws))
        if args.log_every and (i + 1) % args.log_every == 0:
            log(f"iteration {i + 1}/{args.iterations} loss {float(loss.item()):.6f}")
    torch.cuda.synchronize()
    E.save_checkpoint(path, tr.trained_state_dict())
    log(f"Model saved at: {path}")
    return path, tr
