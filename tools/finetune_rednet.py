"""Fine-tunes RedNet on the observation stream tools/build_known_maps.py consumes: drives the project's vector env with the
expert action of `shortest_path_sensor` and takes one Adam step per batch on (rgb, depth) -> semantic12
(ivln_ce_amd.rednet_train.RedNetTrainer: five-output pixel cross-entropy, HIP forward and backward), then writes
{"model_state": state_dict} - the file PredictSemantics.setup reads as data/rednet_mp3d_best_model.pkl.

    python tools/finetune_rednet.py --exp-config <yaml> --steps N --out <file> [--init <ckpt>] [--trainable decoder|all]
                                    [--lr 2e-4] [--ignore-label L] [--augment] [--seed S]
                                    [--class-weights none|median] [--weight-batches K] [--holdout K] [--eval-every N]
                                    [KEY VALUE ...]   (trailing config overrides)

--augment: one random scale / crop / flip / saturation-value record per image and step, applied on the device
(rednet_train.AugmentConfig's defaults, drawn from --seed).  --class-weights median: median-frequency weights from the
first --weight-batches batches of the stream, which are then trained on like the rest.  --holdout K: K further batches are
taken from the stream before training and never trained on; every --eval-every steps (0: never) and at the end one line
{step, holdout_miou, holdout_pixel_acc}.

The observation stream is the backend's (trailing `ENV_BACKEND boxworld`: rgb, depth and labels of one consistent world,
rendered on the device; the default synthetic backend draws labels that are independent of the image).

Prints one JSON line per 10 steps {step, loss, per_scale} and a last one with the mIoU of the final batch."""
import argparse
import itertools
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--exp-config", required=True)
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--init", default=None, help='a checkpoint {"model_state": ...} to start from')
    ap.add_argument("--trainable", choices=("all", "decoder"), default="all")
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--ignore-label", type=int, default=None)
    ap.add_argument("--augment", action="store_true", help="augment every training batch on the device")
    ap.add_argument("--seed", type=int, default=0, help="seed of the augmentation records")
    ap.add_argument("--class-weights", choices=("none", "median"), default="none")
    ap.add_argument("--weight-batches", type=int, default=16, help="batches counted for --class-weights median")
    ap.add_argument("--holdout", type=int, default=0, help="batches set aside before training, evaluated only")
    ap.add_argument("--eval-every", type=int, default=0, help="evaluate the held-out batches every N steps (0: at the end)")
    ap.add_argument("opts", nargs=argparse.REMAINDER)
    a = ap.parse_args(argv)
    if a.steps <= 0:
        ap.error("--steps must be positive")
    if a.weight_batches <= 0 or a.holdout < 0 or a.eval_every < 0:
        ap.error("--weight-batches must be positive, --holdout and --eval-every not negative")
    return a


def load_model(init, device):
    from ivln_ce_amd.rednet import PredictSemantics, RedNet

    model = RedNet(PredictSemantics.CFG)
    if init is not None:
        state = torch.load(init, map_location="cpu")["model_state"]
        if next(iter(state)).split(".")[0] == "module":
            state = {".".join(k.split(".")[1:]): v for k, v in state.items()}
        model.load_state_dict(state)
    return model.to(device).train()


def main(argv=None):
    a = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("finetune_rednet: RedNet trains on the GPU (there is no CPU fallback)")
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from build_known_maps import explore  # (the same observation stream)

    from ivln_ce_amd.config import get_config
    from ivln_ce_amd.envs import construct_envs
    from ivln_ce_amd.rednet_train import AugmentConfig, RedNetTrainer, class_counts, median_frequency_weights

    cfg = get_config(a.exp_config, a.opts or None)
    device = torch.device("cuda", int(cfg.TORCH_GPU_ID))
    trainer = RedNetTrainer(load_model(a.init, device), lr=a.lr, trainable=a.trainable, ignore_label=a.ignore_label,
                            augment=AugmentConfig() if a.augment else None, seed=a.seed)
    envs = construct_envs(cfg, auto_reset_done=True, iterative=False, with_rgb=True)
    batch = None

    def checked(b):
        for key in ("rgb", "depth", "semantic12"):
            if key not in b:
                raise SystemExit(f"finetune_rednet: the observations carry no `{key}`")
        return b

    def keep(b):  # (a batch that outlives the env step that produced it)
        return {key: checked(b)[key].clone() for key in ("rgb", "depth", "semantic12")}

    def report_holdout(step):
        m = trainer.evaluate(holdout)
        print(json.dumps({"step": step, "holdout_miou": m["miou"], "holdout_pixel_acc": m["pixel_acc"]}), flush=True)

    try:
        stream = explore(envs, a.steps + a.holdout, device)
        holdout = [keep(b) for b in itertools.islice(stream, a.holdout)]
        if a.class_weights == "median":
            head = [keep(b) for b in itertools.islice(stream, min(a.weight_batches, a.steps))]
            pixels, present = class_counts(head, trainer.classes, a.ignore_label)
            trainer.class_weights = median_frequency_weights(pixels, present).to(device)
            print(json.dumps({"class_weights": [round(float(x), 6) for x in trainer.class_weights.cpu()],
                              "pixels": pixels.tolist(), "present": present.tolist()}), flush=True)
            stream = itertools.chain(head, stream)
        for t, batch in enumerate(stream):
            loss = trainer.step(checked(batch))
            if t % 10 == 0 or t + 1 == a.steps:
                print(json.dumps({"step": t, "loss": loss, "per_scale": trainer.last_per_scale}), flush=True)
            if holdout and a.eval_every and (t + 1) % a.eval_every == 0 and t + 1 != a.steps:
                report_holdout(t + 1)
        if holdout:
            report_holdout(a.steps)
    finally:
        envs.close()
    m = trainer.evaluate([batch])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    trainer.save(a.out)
    print(json.dumps({"out": a.out, "steps": a.steps, "trainable": a.trainable, "last_batch_miou": m["miou"],
                      "last_batch_pixel_acc": m["pixel_acc"]}), flush=True)


if __name__ == "__main__":
    main()
