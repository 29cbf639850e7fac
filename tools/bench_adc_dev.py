#!/usr/bin/env python3
"""What an int16 device shard (engine.AdcShard) costs against the float32 shard it stands for, on one MI355X.

The C3 parameters of bench.py (10 barcodes x 110-point references, window 15) on a shard small enough that the float32 copy
and the int16 copy both fit (default 2 M reads).  The synthetic reads are quantised ON the device -- per-read scale and
offset as tests/helpers/adc_inputs.py draws them -- and calibrated back by the contract's formula, so that both paths see
identical rows; the results are compared once (status, call, dist) before anything is timed.  In one process `demux` on the
float32 rows and `demux(AdcShard)` alternate; recorded: median ms and spread of each, the decode kernel's own ms and
achieved bytes/s (wdx_kernel_time, from a run of its own with the event brackets on), and the device bytes each shard and
the staging block hold.  Cost model to compare against: int16 path = float32 path + the decode kernel.

    python tools/bench_adc_dev.py --out profiles/adc_dev.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def quantise_on_device(torch, sig, off, chunk_reads=100_000):
    """(adc int16 packed on multiples of 8, offsets int64[n+1], row_len int32, offset, scale); `sig` is overwritten with the
    calibration of the int16 samples, float32 add then float32 multiply, so that it IS the rows the shard stands for"""
    dev = sig.device
    n = off.numel() - 1
    lens = off[1:] - off[:-1]
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    scale = (0.1755 * (1.0 + 0.02 * (2 * torch.rand(n, generator=g, device=dev) - 1))).float()
    offset = (-240.0 + 20.0 * (2 * torch.rand(n, generator=g, device=dev) - 1)).float()
    off16 = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum((lens + 7) // 8 * 8, 0, out=off16[1:])
    adc = torch.zeros(int(off16[-1].item()) + 8, dtype=torch.int16, device=dev)
    for r0 in range(0, n, chunk_reads):
        r1 = min(n, r0 + chunk_reads)
        s0, s1 = int(off[r0].item()), int(off[r1].item())
        rid = torch.repeat_interleave(torch.arange(r0, r1, device=dev), lens[r0:r1])
        x = sig[s0:s1]
        q = torch.clamp(torch.round(x.double() / scale[rid].double() - offset[rid].double()), -32768, 32767).to(torch.int16)
        adc[off16[rid] + (torch.arange(s0, s1, device=dev) - off[rid])] = q
        x.copy_((q.float() + offset[rid]) * scale[rid])
        del rid, q
    return adc, off16, lens.to(torch.int32), offset, scale


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=7, help="alternations after the warm-up (at least 5)")
    ap.add_argument("--slice-reads", type=int, default=0, help="WDX_OPT_ADC_DEV_SLICE_READS (0 = built-in; only lowers the slice)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    import bench
    from warpdemux_amd import _lib, sig_proc, synth
    from warpdemux_amd.engine import AdcShard, DemuxEngine

    reps = max(5, args.reps)
    spec = synth.SynthSpec(n_barcodes=bench.N_BARCODES)
    clean = synth.SynthSpec(n_barcodes=bench.N_BARCODES, noise_sigma=0.25, spikes=False)
    refs = bench.make_refs(clean, synth, sig_proc, 0)
    params = sig_proc.SegParams(barcode_num_events=bench.K_FPT)
    eng = DemuxEngine(refs, bench.WINDOW, bench.PENALTY, params)
    eng.ctx.set_option(_lib.OPT_ADC_DEV_SLICE_READS, max(0, args.slice_reads))
    n = args.reads
    sig, off, a_s, a_e, _, max_len = eng.synth_packed(spec, 0, n)
    adc, off16, row_len, offset, scale = quantise_on_device(torch, sig, off)
    shard = AdcShard(adc, row_len, offset, scale, offsets=off16)
    torch.cuda.synchronize()

    paths = {
        "float32": lambda out: eng.demux(sig, a_s, a_e, offsets=off, max_len=max_len, out=out),
        "int16": lambda out: eng.demux(shard, a_s, a_e, max_len=max_len, out=out),
    }
    res = {k: f(None) for k, f in paths.items()}     # allocates outputs / workspaces / the staging block: the warm-up
    torch.cuda.synchronize()
    identical = all(bool(torch.equal(getattr(res["float32"], f), getattr(res["int16"], f))) for f in ("status", "call", "counts"))
    identical = identical and bool(torch.equal(res["float32"].dist.view(torch.int32), res["int16"].dist.view(torch.int32)))
    ok_reads = int((res["float32"].status == 0).sum().item())

    ms = {k: [] for k in paths}
    for _ in range(reps):
        for k, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            res[k].counts.zero_()
            e0.record()
            f(res[k])
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))

    # the decode kernel alone: one more int16 call with the library's event brackets on
    eng.kernel_time_reset()
    eng.kernel_timing(True)
    paths["int16"](res["int16"])
    torch.cuda.synchronize()
    dec_ms, dec_launches = eng.kernel_time(_lib.K_ADC_DEV_WINDOWS)
    fp_ms, _ = eng.kernel_time(_lib.K_FINGERPRINT)
    eng.kernel_timing(False)
    pad = params.padding
    lens = row_len.to(torch.int64)
    win = (torch.minimum(a_e.to(torch.int64) + pad, lens) - torch.clamp(a_s.to(torch.int64) - pad, min=0)).clamp(min=0)
    win_samples = int(win.sum().item())
    dec_bytes = win_samples * (2 + 4)      # int16 read, float32 written (the rounding to groups of 8 not counted)

    def summary(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 3) for x in v]}

    f32, i16 = summary(ms["float32"]), summary(ms["int16"])
    spread = max(f32["max_ms"] - f32["min_ms"], i16["max_ms"] - i16["min_ms"])
    gap = i16["median_ms"] - f32["median_ms"]
    out = {
        "tool": "tools/bench_adc_dev.py", "device": torch.cuda.get_device_name(0), "reads": n, "reps": reps, "slice_reads_option": max(0, args.slice_reads),
        "max_len": int(max_len), "samples": int(off[-1].item()), "window_samples": win_samples, "reads_ok": ok_reads,
        "results_identical": identical,
        "float32": dict(f32, reads_per_s=n / f32["median_ms"] * 1e3),
        "int16": dict(i16, reads_per_s=n / i16["median_ms"] * 1e3),
        "decode_kernel": {"ms": dec_ms, "launches": dec_launches, "bytes": dec_bytes,
                          "bytes_per_s": dec_bytes / dec_ms * 1e3 if dec_ms > 0 else None,
                          "fingerprint_chain_ms_same_run": fp_ms},
        "cost_model": {"gap_ms": gap, "decode_ms": dec_ms, "gap_minus_decode_ms": gap - dec_ms, "alternation_spread_ms": spread,
                       "gap_explained_by_decode": bool(gap - dec_ms <= spread)},
        "device_bytes": {"float32_shard": sig.numel() * 4 + off.numel() * 8, "int16_shard": shard.nbytes(),
                         "staging_block": eng.adc_staging_bytes(n, max_len),
                         "slices": -(-n // max(1, eng.adc_staging_bytes(n, max_len) // ((int(max_len) + 8 + 7) // 8 * 8 * 4 + 12)))},
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if not identical:
        raise SystemExit("the int16 path and the float32 path disagree")


if __name__ == "__main__":
    main()
