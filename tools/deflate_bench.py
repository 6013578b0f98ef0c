#!/usr/bin/env python3
"""BGZF deflate throughput and compressed size: the GPU encoder (ganon_deflate_bgzf through
native.GpuDeflater) on the formatter's output shape — the config-2 record set (names of 30-45
characters, half reverse; 9.8 M records by default, made by synth/batch.py + synth/fastq.py and
formatted on the device) — and its size against zlib levels 1 and 6 on the same 0xFF00-byte blocks,
there and on the golden FASTQ of config1 (short reads) and longpair. Warm runs; k_deflate alone by
HIP events (median and range over --iters), the whole call (H2D, kernels, compaction, D2H into
page-locked memory) by wall clock. One JSON line, also written to --out.

    python tools/deflate_bench.py [--reads 9800000] [--iters 5] [--zlib-blocks 256] [--out profiles/deflate_bench.json]
"""
import argparse
import gzip
import json
import os
import sys
import time
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
BLOCK = 0xFF00


def zsize(block, level: int) -> int:
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return len(c.compress(block) + c.flush()) + 26


def sizes_vs_zlib(deflater, data, max_blocks: int) -> dict:
    """Member bytes of the first ``max_blocks`` blocks of ``data`` (0: all) against zlib's."""
    mv = memoryview(data)
    n = len(mv) if not max_blocks else min(len(mv), max_blocks * BLOCK)
    blocks = [mv[i:i + BLOCK] for i in range(0, n, BLOCK)]
    _, sizes = deflater.bgzf(np.frombuffer(mv[:n], np.uint8))
    ours = int(sizes.sum())
    z1 = sum(zsize(b, 1) for b in blocks)
    z6 = sum(zsize(b, 6) for b in blocks)
    return {"blocks": len(blocks), "plain_bytes": n, "gpu_bytes": ours, "zlib1_bytes": z1, "zlib6_bytes": z6,
            "gpu_over_zlib1": round(ours / z1, 4), "gpu_over_zlib6": round(ours / z6, 4),
            "gpu_ratio": round(ours / n, 4), "stored_members": int(np.count_nonzero(sizes >= BLOCK))}


def formatter_output(reads: int) -> np.ndarray:
    from genomeanonymizer_amd import native
    from genomeanonymizer_amd.synth.batch import config2_batch
    from genomeanonymizer_amd.synth.fastq import fastq_records
    arr, _ = config2_batch(n_reads=reads, genome=max(60_000_000, reads * 300), seed=2)
    recs = fastq_records(arr, seed=11, name_len=(30, 45), check_bad=False)
    m = native.HipMasker(0)
    f = m.fastq_upload(recs)
    f.run()
    f.sync()
    out = f.download()
    f.free()
    m.close()
    return np.frombuffer(out, np.uint8) if not isinstance(out, np.ndarray) else out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=9_800_000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--zlib-blocks", type=int, default=256, help="blocks of the formatter output compared with zlib")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from genomeanonymizer_amd import native
    text = formatter_output(a.reads)
    d = native.GpuDeflater(0)
    stream, sizes = d.bgzf(text)                       # warm: buffers grown, page-locked blocks cached
    head = gzip.decompress(stream[:int(sizes[:8].sum())].tobytes())
    assert head == text[:len(head)].tobytes()
    d.set_profiling(True)
    kms, wall = [], []
    for _ in range(a.iters):
        t0 = time.perf_counter()
        d.bgzf(text)
        wall.append(time.perf_counter() - t0)
        kms.append(d.kernel_ms())
    d.set_profiling(False)
    nb = len(text)
    k_med, w_med = float(np.median(kms)), float(np.median(wall))
    res = {
        "reads": a.reads, "plain_bytes": nb, "bytes_per_record": round(nb / a.reads, 1), "members": len(sizes),
        "compressed_bytes": int(sizes.sum()), "iters": a.iters,
        "k_deflate_ms": {"median": round(k_med, 3), "min": round(min(kms), 3), "max": round(max(kms), 3)},
        "k_deflate_input_GB_per_s": round(nb / k_med / 1e6, 3),
        "call_s": {"median": round(w_med, 4), "min": round(min(wall), 4), "max": round(max(wall), 4)},
        "call_input_GB_per_s": round(nb / w_med / 1e9, 3),
        "note": "k_deflate: the encoder kernel alone, HIP events summed over the call's chunks; call: "
                "ganon_deflate_bgzf with host buffers (pageable in, page-locked out), H2D + kernels + D2H, not overlapped",
        "size": {"formatter_output": sizes_vs_zlib(d, text, a.zlib_blocks)},
    }
    for name in ("config1", "longpair"):
        g = os.path.join(REPO, "tests", "golden", name, "normal.1.fastq.gz")
        res["size"][name] = sizes_vs_zlib(d, gzip.open(g).read(), 0)
    d.close()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
