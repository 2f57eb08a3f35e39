"""The child process of tests/test_gpu_stream_order.py::test_torch_recipe_in_a_child_process: the recipe of INTEGRATION.md
section 3 (VoxBox.from_torch) with torch's own work around the call and no host wait in between.  The producer is torch work on
the current stream that ENDS by writing the audio tensor; the consumer is a torch clone of the records.  Run once with a
torch.cuda.Stream current; with torch's default stream current from_torch must refuse (see its docstring).  Prints one JSON line."""
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, H, F, SR = 1200, 480, 300, 48000.0


def recipe(torch, pkg, src, by_hand=False):
    """Inside whatever stream is current: (records equal the synchronised call's, the host was ahead, the context's handle).
    by_hand: the recipe INTEGRATION.md used to give, the handle torch reports passed on as it is."""
    stream = torch.cuda.current_stream()
    vb = pkg.VoxBox(0, stream.cuda_stream) if by_hand else pkg.VoxBox.from_torch()
    try:
        prm = pkg.AnalysisParams.make(SR)
        w = int(vb.L.vbx_record_doubles(C.byref(prm)))
        ld = w + (w & 1)
        # the synchronised call (it also builds the tables and sizes the workspaces)
        audio = src.clone()
        rec = torch.zeros((F, ld), dtype=torch.float64, device=src.device)
        torch.cuda.synchronize()
        vb.analyze_frames(audio, prm, frame_len=N, stride=H, n_frames=F, out=rec, record_ld=ld)
        vb.sync()
        torch.cuda.synchronize()
        ref = rec.clone()
        torch.cuda.synchronize()
        # queued: a few dozen milliseconds of matrix products, then the audio, then the call, then the clone
        a = torch.randn((4096, 4096), dtype=torch.float32, device=src.device)
        audio.fill_(float("nan"))
        rec.fill_(float("nan"))
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        b = a
        for _ in range(40):
            b = (a @ b) * (1.0 / 64.0)
        t1.record()
        audio.copy_(src + 0.0 * b[0, 0].to(torch.float64))            # the producer's last step depends on everything before it
        vb.analyze_frames(audio, prm, frame_len=N, stride=H, n_frames=F, out=rec, record_ld=ld)
        got = rec.clone()
        host_ahead = not stream.query()
        stream.synchronize()
        torch.cuda.synchronize()
        delay_ms = t0.elapsed_time(t1)
        same = bool(torch.equal(got.view(torch.int64), ref.view(torch.int64))) and bool(torch.isfinite(ref[:, :2]).all())
        return {"equal": same, "host_ahead": bool(host_ahead), "delay_ms": round(delay_ms, 2),
                "handle": int(stream.cuda_stream), "context_handle": int(vb.stream_handle)}
    finally:
        vb.sync()
        vb.close()


def main():
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    torch.cuda.set_device(0)
    n = (F - 1) * H + N
    t = torch.arange(n, dtype=torch.float64, device="cuda") / SR
    gen = torch.Generator(device="cpu").manual_seed(7)
    noise = torch.randn(n, generator=gen, dtype=torch.float64).to("cuda")
    src = 0.5 * torch.sin(2 * math.pi * 140.0 * t) + 0.3 * torch.sin(2 * math.pi * 281.0 * t) + 0.2 * torch.sin(2 * math.pi * 2400.0 * t) + 0.01 * noise
    torch.cuda.synchronize()
    out = {}
    with torch.cuda.stream(torch.cuda.Stream()):
        out["stream"] = recipe(torch, pkg, src)
    torch.cuda.synchronize()
    # torch's default stream current: its handle is 0, which the C ABI reads as "own stream"; from_torch refuses it
    handle = int(torch.cuda.current_stream().cuda_stream)
    try:
        pkg.VoxBox.from_torch().close()
        out["default_stream"] = {"handle": handle, "refused": False, "message": ""}
    except pkg.VoxBoxError as e:
        out["default_stream"] = {"handle": handle, "refused": True, "message": str(e)}
    # what from_torch refuses, done by hand once: a context on a stream of its own, beside torch's work (recorded, a race)
    out["handle_0_passed_by_hand"] = recipe(torch, pkg, src, by_hand=True)
    print(json.dumps(out))                                   # the parent asserts on it
    return 0


if __name__ == "__main__":
    sys.exit(main())
