"""Per-layer cost of capturing a ViT teacher's attention for the loss, three ways, on one attention block:
  reference  the reference hook (``make_attn_capture_hook(cls_row_only=False)``): second qkv projection, full N x N map
  cls_row    the CLS-row torch path (``cls_row_only=True``): q of the CLS token and k of every token, projected again
             (teachers with a CLS token only)
  fused      ``make_qkv_importance_hook`` on the block's own qkv Linear: one launch of ``basd_attn_importance``
Each is the time of the attention module's forward WITH the hook minus the time of the forward without any hook, so the
block's own projection and attention are not counted; peak allocated memory is the capture's own (over the same forward
without a hook).  Shapes: ViT-B (N = 197 with CLS, 196 without, H = 12) at B = 256 and ViT-L (N = 197, H = 16) at
B = 128, fp32 and bf16.
usage: attn_capture_bench.py [--iters 20] [--out profiles/attn_capture.txt]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-inductive-bias-distillation_amd"))
import torch
from basd_amd import capture
from tools import stock_models as SM

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_capture.txt"))
args = ap.parse_args()
dev = torch.device("cuda", 0)

CASES = [("ViT-B", 768, 12, 197, True, 256), ("ViT-B", 768, 12, 196, False, 256), ("ViT-L", 1024, 16, 197, True, 128)]


def measure(fn, iters):
    """(median ms of ``fn``, peak bytes allocated over the state before the call)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2], peak


lines = [f"# attn_capture_bench.py --iters {args.iters}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
         "# ms = median time of the attention module's forward with the hook minus the same forward without a hook;",
         "# MiB = peak allocated memory of the hooked forward minus that of the plain forward (the capture's own)",
         f"{'model':6} {'N':>4} {'cls':>4} {'B':>4} {'dtype':>5} {'path':>10} {'fwd ms':>8} {'hook ms':>8} {'hook MiB':>9}"]
for name, dim, heads, N, has_cls, B in CASES:
    for dtype in (torch.float32, torch.bfloat16):
        torch.manual_seed(0)
        attn = SM._Attention(dim, heads).to(dev).to(dtype).eval()
        x = torch.randn(B, N, dim, device=dev, dtype=dtype)
        store = {}

        @torch.no_grad()
        def forward():
            store.clear()
            attn(x)

        plain_ms, plain_peak = measure(forward, args.iters)
        paths = [("reference", lambda: attn.register_forward_hook(capture.make_attn_capture_hook(store, 0)))]
        if has_cls:
            paths.append(("cls_row", lambda: attn.register_forward_hook(
                capture.make_attn_capture_hook(store, 0, cls_row_only=True))))
        paths.append(("fused", lambda: attn.qkv.register_forward_hook(capture.make_qkv_importance_hook(
            store, 0, heads, mode="cls_row" if has_cls else "query_mean"))))
        for label, register in paths:
            handle = register()
            ms, peak = measure(forward, args.iters)
            handle.remove()
            lines.append(f"{name:6} {N:4d} {str(has_cls):>4} {B:4d} {str(dtype).split('.')[1][:5]:>5} {label:>10} "
                         f"{plain_ms:8.3f} {ms - plain_ms:8.3f} {(peak - plain_peak) / 2**20:9.1f}")
            print(lines[-1], flush=True)
        del attn, x
        torch.cuda.empty_cache()
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
print(text)
