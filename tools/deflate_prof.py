"""Where k_deflate's cycles go (tuning): run with a -DDEF_PROF build of libganon_hip.so
(tools/build_variant.py defprof -DDEF_PROF; GANON_HIP_LIB=<that .so>) over the golden config1 FASTQ
repeated to about 100 MB; prints lane 0's summed s_memtime cycles per phase (stage + crc, match +
greedy parse, code construction, token bit lengths, emit + store), per input byte and as shares."""
import ctypes as C
import gzip
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    from genomeanonymizer_amd import native
    text = gzip.open(os.path.join(REPO, "tests", "golden", "config1", "normal.1.fastq.gz")).read()
    big = np.tile(np.frombuffer(text, np.uint8), -(-100_000_000 // len(text)))
    d = native.GpuDeflater(0)
    fn = native.hip_lib().ganon_deflate_prof_read
    buf = (C.c_ulonglong * 5)()
    d.bgzf(big)
    fn(buf)
    d.bgzf(big)
    fn(buf)
    names = ["stage_crc", "match_parse", "codes", "token_bits", "emit_store"]
    tot = sum(int(v) for v in buf)
    res = {"input_bytes": len(big), "cycles": {n: int(v) for n, v in zip(names, buf)},
           "per_input_byte": {n: round(int(v) / len(big), 3) for n, v in zip(names, buf)},
           "share": {n: round(int(v) / max(1, tot), 3) for n, v in zip(names, buf)},
           "note": "s_memtime ticks of lane 0 of every block's workgroup, summed over the blocks"}
    print(json.dumps(res))
    d.close()


if __name__ == "__main__":
    main()
