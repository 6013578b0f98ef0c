#!/usr/bin/env python3
"""Golden fixtures for ``--masked_base_quality``: run the UNMODIFIED reference with its own
quality hook switched on and store its outputs under ``tests/golden/maskq2/<scenario>/``.

``AnonymizedRead.mask_or_modify_base_pair(pos, base, modify_qualities=False, new_quality=0)``
already writes ``new_quality`` at the masked position when asked to; the reference never asks.
This tool wraps that one method so that every call passes ``modify_qualities=True,
new_quality=Q`` (Q=2, '#') and otherwise runs ``oracle/run_reference.py`` as it stands: same
entry point, same scenarios, same file layout and ``meta.json``. Only the reference's output
data is kept; the wrapper below is this project's code.

The reference's modules are imported inside ``run_reference``, so one scenario is run unhooked
into a scratch directory first and the class is then patched in ``sys.modules``.

Scenarios the hooked reference cannot finish (it raises ``TypeError: 'reversed' object does
not support item assignment`` when the hook meets a record that was already formatted once)
are reported and get no fixture.

usage: python tools/make_maskq_golden.py [scenario ...]
"""
from __future__ import annotations

import importlib.util
import json
import os
import shutil
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALITY = 2
SCENARIOS = ["tiny", "edge", "fuzz9", "fuzz1001", "fuzz3000", "long1", "fuzz2000", "fuzz2003"]


def _load_run_reference():
    spec = importlib.util.spec_from_file_location(
        "ganon_run_reference", os.path.join(REPO, "oracle", "run_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def hook_reference(rr, quality: int = QUALITY):
    """Import the reference (by one unhooked run) and switch its quality hook on."""
    scratch = tempfile.mkdtemp(prefix="ganon_maskq_warm_")
    try:
        rr.run_reference("tiny", scratch)
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    am = sys.modules["src.GenomeAnonymizer.anonymizer_methods"]
    plain = am.AnonymizedRead.mask_or_modify_base_pair
    if getattr(plain, "_maskq_hooked", False):
        return

    def hooked(self, pos_in_read, new_base, modify_qualities=False, new_quality=0):
        return plain(self, pos_in_read, new_base, True, quality)

    hooked._maskq_hooked = True
    am.AnonymizedRead.mask_or_modify_base_pair = hooked


def main(names):
    rr = _load_run_reference()
    hook_reference(rr)
    root = os.path.join(REPO, "tests", "golden", "maskq%d" % QUALITY)
    os.makedirs(root, exist_ok=True)
    for name in names:
        stage = tempfile.mkdtemp(prefix="ganon_maskq_stage_")
        try:
            m = rr.run_reference(name, stage)
        except TypeError as e:
            print(json.dumps({"scenario": name, "raises": "TypeError: %s" % e}))
            continue
        finally:
            if not os.path.isdir(os.path.join(stage, name)):
                shutil.rmtree(stage, ignore_errors=True)
        dest = os.path.join(root, name)
        shutil.rmtree(dest, ignore_errors=True)
        shutil.move(os.path.join(stage, name), dest)
        shutil.rmtree(stage, ignore_errors=True)
        print(json.dumps({"scenario": name, "seconds": m["reference_seconds"],
                          "files": sorted(m["outputs_sha256"])}))


if __name__ == "__main__":
    main(sys.argv[1:] or SCENARIOS)
