#!/usr/bin/env python3
"""Profiling driver for the FASTQ formatter alone: config-2 record set (10 M reads, names of
30-45 characters, half reverse), uploaded from host buffers, formatted RUNS times, the
kernel times printed as one JSON line. Usage: python3 tools/fq_run.py [--reads N] [--runs R]
With --masked_base_quality Q every record also gets an original (a second copy of the bases that
differs in about one base per kb, as germline SNV masks would leave it) and the same runs are timed
once more with the option on: "kernel_ms_maskq" holds k_fq_maskq beside the formatter's kernels."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--configs", default="0:0",
                    help="comma list of kd:skip (GANON_PARAM_FASTQ_KD / _SKIP), timed interleaved")
    ap.add_argument("--masked_base_quality", type=int, default=None, metavar="Q",
                    help="also time the runs with the option on (k_fq_maskq after the formatter)")
    a = ap.parse_args()
    import numpy as np
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.synth.batch import config2_batch
    from genomeanonymizer_amd.synth.fastq import fastq_records
    arr, _ = config2_batch(n_reads=a.reads, genome=max(60_000_000, a.reads * 300), seed=2)
    recs = fastq_records(arr, seed=11, name_len=(30, 45), check_bad=False)
    m = native.HipMasker(0)
    f = m.fastq_upload(recs)
    f.run()
    f.sync()
    cfgs = [tuple(int(x) for x in c.split(":")) for c in a.configs.split(",")]

    def timed(h):
        m.set_profiling(True)
        per = {c: [] for c in cfgs}
        for _ in range(a.runs):
            for c in cfgs:
                m.set_param(native.PARAM_FASTQ_KD, c[0])
                m.set_param(native.PARAM_FASTQ_SKIP, c[1])
                h.run()
                h.sync()
                per[c].append({k: ms for k, _, ms in h.kernel_times()})
        m.set_profiling(False)
        return per
    med = lambda per: {f"{c[0]}:{c[1]}": {k: round(float(np.median([t[k] for t in ts])), 4) for k in ts[0]}
                       for c, ts in per.items()}
    per = timed(f)
    maskq = None
    if a.masked_base_quality is not None:
        rng = np.random.default_rng(5)
        orig = recs["seq_bufs"][0].copy()
        at = rng.integers(0, len(orig), len(orig) // 500)
        orig[at] ^= 0x30            # the byte's first base gets another code: about one base per kb differs
        mq = dict(recs, seq_bufs=[recs["seq_bufs"][0], orig], maskq=a.masked_base_quality,
                  orig_sel=np.ones(len(recs["seq_len"]), np.uint8), orig_nib_off=recs["seq_nib_off"].copy())
        g = m.fastq_upload(mq)
        g.run()
        g.sync()
        maskq = med(timed(g))
        plain = f.download()
        patched = g.download()
        maskq["characters_patched"] = int((np.frombuffer(plain, np.uint8) != np.frombuffer(patched, np.uint8)).sum())
        g.free()
    m.set_param(native.PARAM_FASTQ_KD, cfgs[0][0])
    m.set_param(native.PARAM_FASTQ_SKIP, 0)
    times = per[cfgs[0]]
    t = time.perf_counter()
    for _ in range(a.runs):
        f.run()
    f.sync()
    wall = (time.perf_counter() - t) / a.runs * 1e3
    out = f.download()
    ok = len(out) == native.fastq_bytes(recs)
    f.free()
    print(json.dumps({"reads": a.reads, "bytes": len(out), "ok": ok, "wall_ms": round(wall, 4),
                      "kernel_ms": med(per), "kernel_ms_maskq": maskq}))


if __name__ == "__main__":
    main()
