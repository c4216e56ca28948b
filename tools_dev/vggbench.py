"""Microbench: LPIPS VGG16 taps forward (64 images) and forward+backward (32 images) at 256^2,
HIP implicit-GEMM stack (torch_utils/ops/vgg_hip.py) vs MIOpen (VFM_LPIPS_VGG=torch path).
`--forms`: only the per-layer-shape table of the conv kernel's two forms (tiled / patch-staged), see forms_table."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vfm-vae_amd"), ROOT]
import torch

from training.lpips import vgg16
from torch_utils.ops import kernel_timer

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")


def bench(fn, iters=5):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def forms_table(rounds=3, iters=5):
    """`--forms`: time per LPIPS VGG16 conv layer shape of the training step (forward over the 64-image pair batch,
    data gradient over 32 images; Cin >= 32) and per kernel form of vfm_conv3x3_nhwc_f32_form (1 = tiled, 2 =
    patch-staged), the forms alternating in one process over `rounds` rounds of `iters` launches on random data;
    the outputs of the two forms are compared bit for bit on the way."""
    from torch_utils import custom_ops
    from torch_utils.ops import vgg_hip
    lib = custom_ops.get_native()
    chans = [(64, 64, 256), (64, 128, 128), (128, 128, 128), (128, 256, 64), (256, 256, 64), (256, 512, 32),
             (512, 512, 32), (512, 512, 16)]
    shapes = [("fwd", 64, hw, ci, co) for ci, co, hw in chans] + [("dgrad", 32, hw, co, ci) for ci, co, hw in chans]
    g = torch.Generator(device="cuda").manual_seed(0)
    print(f"{'layer':>6s} {'B':>3s} {'HxW':>4s} {'Cin':>4s} {'Cout':>4s} | " + " ".join(
        f"{f'r{k} tiled':>9s} {f'r{k} patch':>9s}" for k in range(rounds)) + " |  tiled us  patch us  patch/tiled   TF/s tiled -> patch  equal")
    tot = {1: 0.0, 2: 0.0}
    for kind, B, hw, cin, cout in shapes:
        x = torch.randn(B, hw, hw, cin, generator=g, device="cuda")
        w = vgg_hip.split_weight(torch.randn(cout, 9 * cin, generator=g, device="cuda") * (9 * cin) ** -0.5, 3)
        bias = torch.randn(cout, generator=g, device="cuda")
        mask = torch.randn(B, hw, hw, cout, generator=g, device="cuda") if kind == "dgrad" else None
        outs = {f: torch.empty(B, hw, hw, cout, device="cuda") for f in (1, 2)}

        def run(form):
            rc = lib.vfm_conv3x3_nhwc_f32_form(x.data_ptr(), w.data_ptr(), custom_ops.VFM_F32, w.shape[2],
                                               None if mask is not None else bias.data_ptr(), custom_ops.ptr(mask),
                                               outs[form].data_ptr(), B, hw, hw, cin, cout, int(mask is None),
                                               custom_ops.stream_ptr(x.device), form)
            custom_ops.check(rc, "vfm_conv3x3_nhwc_f32_form")

        for f in (1, 2):
            run(f)
        torch.cuda.synchronize()
        same = torch.equal(outs[1], outs[2])
        ts = {1: [], 2: []}
        for _ in range(rounds):
            for f in (1, 2):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(iters):
                    run(f)
                e.record()
                torch.cuda.synchronize()
                ts[f].append(s.elapsed_time(e) / iters * 1e3)
        m = {f: sum(v) / len(v) for f, v in ts.items()}
        for f in (1, 2):
            tot[f] += m[f]
        fl = 2.0 * B * hw * hw * cout * 9 * cin
        print(f"{kind:>6s} {B:3d} {hw:4d} {cin:4d} {cout:4d} | " + " ".join(
            f"{ts[1][k]:9.1f} {ts[2][k]:9.1f}" for k in range(rounds)) +
            f" | {m[1]:9.1f} {m[2]:9.1f} {m[2] / m[1]:12.3f}   {fl / m[1] / 1e6:10.1f} -> {fl / m[2] / 1e6:6.1f}  {same}",
            flush=True)
    print(f"sum over the shapes: tiled {tot[1] / 1e3:.2f} ms, patch {tot[2] / 1e3:.2f} ms")


if "--forms" in sys.argv:
    forms_table()
    sys.exit(0)

net = vgg16(pretrained=False).cuda()
x64 =torch.randn(64, 3, 256, 256, device="cuda")
x32 = torch.randn(32, 3, 256, 256, device="cuda", requires_grad=True)
GF = 2 * 20.1e9 * 1.0          # conv flops per image forward (sum over the 13 layers)
for impl in ("hip", "torch"):
    type(net).impl = impl
    with torch.no_grad():
        tf = bench(lambda: net(x64))

    def fb():
        outs = net(x32)
        torch.autograd.backward(list(outs), [torch.ones_like(o) for o in outs])

    tb = bench(fb)
    print(f"{impl:6s} fwd 64 img {tf:7.2f} ms ({64 * GF / tf / 1e9:6.1f} TF/s)   fwd+bwd 32 img {tb:7.2f} ms", flush=True)
type(net).impl = "hip"
kernel_timer.enable(True)
with torch.no_grad():
    net(x64)
for k, v in sorted(kernel_timer.summary().items(), key=lambda kv: -kv[1]["total_ms"]):
    print(f"  {k:40s} {v['total_ms']:7.3f} ms  {v['flops'] / v['total_ms'] / 1e9:7.1f} TF/s")

# kernel breakdown of one HIP forward + backward (32 images)
from torch.profiler import profile, ProfilerActivity
type(net).impl = "hip"
fb()
torch.cuda.synchronize()
with profile(activities=[ProfilerActivity.CUDA]) as prof:
    fb()
    torch.cuda.synchronize()
print(prof.key_averages().table(sort_by="self_cuda_time_total", row_limit=25, max_name_column_width=70))
