"""Time the layer2 resident-weight conv (variant 41, csrc/l2conv.hip) in its
three inference forms -- plain (conv1 of layer2.1), res (conv2 + identity as
an epilogue residual), ds (layer2.0's conv2 + the 1x1/2 downsample) -- on
N-image batches of 64 x 64 x 128 bf16 maps, the bench's layer2 shape.  10
back-to-back launches x 3 (median) after warm-up; us per launch and TFLOP/s
of the form's algorithmic work.

  --n N ...        batch sizes (default 1024: one launch of the bench's step)
  --ablate A ...   also time the timing-ablation kernels (wrong results):
                   8 no output stores, 32 no patch DMA in the tile loop
  --digest         instead of timing: SHA-256 of the outputs of
                   tests/test_gpu_l2conv_loop.py's cases, one line per case,
                   to compare two builds of the library bit for bit
"""
import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'synthetic-audio-detection_amd'))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))
import torch  # noqa: E402

DEV = 'cuda:0'
FORMS = ('plain', 'res', 'ds')


def timeit(fn, iters=10, reps=3):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1000.0 / iters)
    return sorted(ts)[len(ts) // 2]


def operands(form, n, hw=64):
    g = torch.Generator(device=DEV).manual_seed(41)
    cin1 = 64 if form == 'ds' else 0
    K = 9 * 128 + cin1
    x = torch.randn(n, hw, hw, 128, generator=g, device=DEV).to(torch.bfloat16)
    w = (torch.randn(128, K, generator=g, device=DEV) * (2.0 / K) ** 0.5).to(torch.bfloat16)
    bias = torch.randn(128, generator=g, device=DEV) * 0.1
    sc = torch.randn(n, 2 * hw, 2 * hw, 64, generator=g, device=DEV).to(torch.bfloat16) if form == 'ds' else None
    res = torch.randn(n, hw, hw, 128, generator=g, device=DEV).to(torch.bfloat16) if form == 'res' else None
    return x, w, bias, sc, res, torch.empty(n, hw, hw, 128, device=DEV, dtype=torch.bfloat16)


def run(ops, ablate=0):
    from sad.engine import block_conv
    x, w, bias, sc, res, out = ops
    return block_conv(x, w, bias, 1, 1, sc=sc, sc_stride=2 if sc is not None else 1, relu=True,
                      variant=41 | (ablate << 8), res=res, out=out)


def digest():
    import test_gpu_l2conv_loop as t
    for form, N, H, W, relu in t.cases():
        out = t.launch(form, N, H, W, relu)
        h = hashlib.sha256(out.view(torch.int16).cpu().numpy().tobytes()).hexdigest()
        print(f'{form}-{N}x{H}x{W}{"" if relu else "-norelu"} {h}', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, nargs='+', default=[1024])
    ap.add_argument('--ablate', type=int, nargs='*', default=[])
    ap.add_argument('--digest', action='store_true')
    args = ap.parse_args()
    if args.digest:
        return digest()
    for n in args.n:
        for form in FORMS:
            ops = operands(form, n)
            fl = 2.0 * n * 64 * 64 * 128 * (9 * 128 + (64 if form == 'ds' else 0))
            t = timeit(lambda: run(ops))
            print(f'N={n} {form}: {t:.1f} us ({fl / t / 1e6:.0f} TFLOP/s)', flush=True)
            for ab in args.ablate:
                ta = timeit(lambda: run(ops, ab))
                print(f'  ablate {ab}: {ta:.1f} us', flush=True)
            del ops
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
