#!/usr/bin/env python3
"""ESD (the reference's baselines/erasing/esd_diffusers.py with its flags): fine-tune some modules of the pruned checkpoint
so that it no longer draws a concept.
    python scripts/baselines/erasing/esd_diffusers.py --erase_concept "Van Gogh" --train_method xattn \\
        --base_config_path CFG --model_id <SD-2.1 snapshot> --ckpt_path <pruned>/checkpoint-N/

* --erase_concept / --erase_from: comma-separated; one erase_from serves every concept, none means the concept itself.
* --train_method: xattn (every attn2 Linear), noxattn (every other Linear / Conv2d), selfattn (every attn1 Linear);
  xattn-strict selects nothing and raises ValueError like torch.optim.Adam on an empty list; anything else (the help text's
  `full` included) raises NotImplementedError.  Norms are never trained.
* Per iteration: a pair, an `iteration` in 1 ... 48 and 64 x 64 latents are drawn on the host generators (seeded once by
  --seed), `iteration` DDIM steps of 50 at guidance 3 with the fine-tuned weights (--graph 1: the captured loop), the frozen
  predictions for the concept, '' and erase_from, and one Adam step on mse(student(erase_from), e_f - ng (e_p - e_n)).
* Writes <--save_path>/esd-<concept>_from_<from>-<method>_<ng>-epochs_<iterations>.pt: {"unet.<module>": {"weight", "bias"}}
  of the trained modules, fp32 - what `artist_erasure.py --baseline esd --ckpt_name` and `generate_fid_images.py
  --erasure_ckpt_path` load.
"""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="TrainESD", description="Finetuning stable diffusion to erase the concepts")
    p.add_argument("--erase_concept", help="concept to erase", type=str, required=True)
    p.add_argument("--erase_from", help="target concept to erase from", type=str, required=False, default=None)
    p.add_argument("--train_method", help="Type of method (xattn, noxattn, selfattn, xattn-strict)", type=str, required=True)
    p.add_argument("--iterations", help="Number of iterations", type=int, default=1000)
    p.add_argument("--lr", help="Learning rate", type=float, default=1e-5)
    p.add_argument("--negative_guidance", help="Negative guidance value", type=float, required=False, default=1)
    p.add_argument("--save_path", help="Path to save model", type=str, default="models/")
    p.add_argument("--device", help="cuda device to train on", type=str, required=False, default="cuda:0")
    p.add_argument("--base_config_path", help="Path to base config file", type=str, required=False)
    p.add_argument("--ckpt_path", help="Path to checkpoint file", type=str, required=False)
    # not in the reference
    p.add_argument("--model_id", help="local SD-2.1 snapshot (overrides the config's pretrained_model_name_or_path)", type=str,
                   default=None)
    p.add_argument("--tiny", help="tiny topology (tests)", action="store_true")
    p.add_argument("--seed", help="seeds numpy and torch once (the reference is unseeded)", type=int, default=0)
    p.add_argument("--image_size", help="image side; the latents are an eighth of it", type=int, default=512)
    p.add_argument("--mixed_precision", help="no (fp32 like the reference's pipeline) or bf16", choices=("no", "bf16"),
                   default="no")
    p.add_argument("--graph", help="1: partial sampling as replays of a captured graph, 0: eager", type=int, choices=(0, 1),
                   default=1)
    p.add_argument("--log_every", help="read the loss back every N iterations (0: never)", type=int, default=100)
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(levelname)s %(message)s")
    from pdm.utils import esd as E
    E.check_train_method(args.train_method)
    from pdm.training.esd import train
    return train(args)[0]


if __name__ == "__main__":
    main()
