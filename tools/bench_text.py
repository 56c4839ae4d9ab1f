"""Text-encoder timings on the device -> profiles/text_encoder_bench.txt.

For 1, 2 and 24 DISTINCT prompts, both Stable-Diffusion text-tower shapes (1024 / 23 layers / gelu, 768 / 12 layers / quick_gelu; seeded random weights -- no
checkpoints exist offline):
  (a) transformers' CLIPTextModel on the device, one prompt per call: what FreeFinePipeline._encode_text does with a torch encoder;
  (b) freefine_amd.text.HipCLIPTextEncoder, all prompts in one call, in fp32, split-bf16 and bf16.
Device-event times of warmed calls (every shape run --warmup times first: code objects loaded, library algorithms and the bf16 tuner settled), the median
and the spread of --reps calls.  A report, not a gate: the text encoder is about 2 % of an edit step and its embeddings are cached per prompt.

    python tools/bench_text.py [--out profiles/text_encoder_bench.txt] [--reps 20] [--warmup 3]
    python tools/bench_text.py --trace-only --dim 768 --mode x3      # a few native calls and nothing else: the program of a kernel-trace run
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def tokens(n, vocab=49408, S=77):
    """n distinct token rows of realistic layout: BOS, 3 .. 20 word ids, EOS padding"""
    g = torch.Generator().manual_seed(n)
    ids = torch.full((n, S), vocab - 1, dtype=torch.int64)
    ids[:, 0] = vocab - 2
    for i in range(n):
        k = 3 + (5 * i) % 18
        ids[i, 1:1 + k] = torch.randint(0, vocab - 2, (k,), generator=g)
    return ids


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_encoder_bench.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--mode", default="x3", choices=["f32", "x3", "bf16"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_text.py measures on the GPU: none visible")
    from freefine_amd.text import HipCLIPTextEncoder, clip_shaped_text_encoder
    dev = torch.device("cuda:0")
    modes = {"f32": (torch.float32, False), "x3": (torch.float32, True), "bf16": (torch.bfloat16, False)}
    if a.trace_only:
        enc = clip_shaped_text_encoder(a.dim)
        nat = HipCLIPTextEncoder.from_torch(enc, dtype=modes[a.mode][0], device=dev, x3=modes[a.mode][1])
        for n in (1, 2, 24):
            for _ in range(3):
                nat(tokens(n))
        torch.cuda.synchronize()
        return
    lines = [f"text encoder, device-event ms per request of n distinct prompts: median [min .. max] of {a.reps} warmed calls ({torch.cuda.get_device_name(0)})",
             "(a) transformers CLIPTextModel on the device, one prompt per call (fp32 library GEMMs); (b) HipCLIPTextEncoder, one call, groups of "
             f"{HipCLIPTextEncoder.GROUP} prompts", ""]
    for dim in (1024, 768):
        enc = clip_shaped_text_encoder(dim)
        cfg = enc.config
        lines.append(f"width {dim}, {cfg.num_hidden_layers} layers, {cfg.num_attention_heads} heads, MLP {cfg.intermediate_size}, {cfg.hidden_act}")
        rows = {}
        nats = {m: HipCLIPTextEncoder.from_torch(enc, dtype=dt, device=dev, x3=x3) for m, (dt, x3) in modes.items()}
        enc = enc.to(dev)
        for n in (1, 2, 24):
            ids = tokens(n)
            idd = ids.to(dev)
            with torch.no_grad():
                rows[("(a) transformers, per prompt", n)] = timed(lambda: [enc(idd[j:j + 1])[0] for j in range(n)], a.reps, a.warmup)
            for m, nat in nats.items():
                rows[(f"(b) native {m}", n)] = timed(lambda: nat(ids), a.reps, a.warmup)
        for name in ["(a) transformers, per prompt"] + [f"(b) native {m}" for m in modes]:
            lines.append(f"  {name:30s}" + "".join(f"   n={n:2d}: {rows[(name, n)][0]:8.3f} [{rows[(name, n)][1]:7.3f} .. {rows[(name, n)][2]:7.3f}]" for n in (1, 2, 24)))
        lines.append("")
        del enc, nats
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
