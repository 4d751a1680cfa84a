"""Which subset of the INT8 form of BASELINE configs[4] (rr_config.fp8 with "q8_format" = 1: W8A8 QKV / FFN-up, LayerNorm gains
migrated into the weights) ranks like the fp32 reference?  The device study behind the int8 default of "fp8_first_layer"
(rr_api.hip INT8_SAFE_LAYERS, DESIGN.md "int8").  For every committed c5 ranking fixture and every configuration

    fp8_first_layer k   (text-encoder layers below k keep 16-bit operands)
  x q8_smooth 1 | 0     (0: plain per-channel int8, no gain migration; whole stack only)

it prints / records |dlogit| (max and centred per list), rank correlation, top-5 overlap, whether the top-5 SET is kept, whether
the rule binds on the list (the reference's autocast keeps its top-5 with max |d| <= gap / 4) and, per configuration, the verdict
"ranks with margin" (every binding list keeps the top-5 with centred drift <= gap / 2).  Test infrastructure.

    python tests/tools/int8_subset_study.py [--json int8_subset_study.json] [--fixtures ...] [--first-layers ...]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rmr_amd  # noqa: E402
from rmr_amd import _lib  # noqa: E402
from helpers import GOLDEN, arch_from_cfg, load_fullsize, margin_stats, ranking_yardstick, top5_set  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default="int8_subset_study.json", help="where the records go (relative: to the working directory)")
ap.add_argument("--fixtures", default="c5_sep,c5_sep_wide,c5_sep_g20,c5_sep_g15")
ap.add_argument("--first-layers", default="0,6,12,16,18,20,22,23")
a = ap.parse_args()
ks = [int(v) for v in a.first_layers.split(",")]
lib = _lib.load()
out, verdict = {}, {}


def engine(cfg, vision, w, smooth):
    assert lib.rr_set_tuning(b"q8_smooth", smooth) == 0
    try:
        arch = arch_from_cfg(cfg, vision, "fp16")
        arch["fp8"] = 1
        arch["q8_format"] = 1
        eng = rmr_amd.RerankEngine(arch)
        eng.load_state_dict(w)                     # the smoothing is folded here
    finally:
        lib.rr_set_tuning(b"q8_smooth", 1)
    return eng


for name in a.fixtures.split(","):
    if not os.path.exists(os.path.join(GOLDEN, f"{name}.npz")):
        print(f"[{name}] fixture not present, skipped")
        continue
    cfg, w, vision, qs = load_fullsize(name)
    ys = [ranking_yardstick(q) for q in qs]
    for qi, y in enumerate(ys):
        print(f"[{name} q{qi}] gap {y['gap']:.3f} | reference bf16-autocast: |d| {y['stats']['max_abs']:.3e} centred "
              f"{y['stats']['centred']:.3e} -> the rule {'BINDS' if y['binds'] else 'does not bind'} here", flush=True)
    for smooth, firsts in ((1, ks), (0, [0])):
        eng = engine(cfg, vision, w, smooth)
        for k in firsts:
            eng.set_option("fp8_first_layer", k)
            tag = f"int8_first{k}_smooth{smooth}"
            line = []
            for qi, (q, y) in enumerate(zip(qs, ys)):
                sel, ref = y["sel"], y["ref"]
                r = eng.forward_ids(q["ids"][sel].cuda(), q["am"][sel].cuda(), q["tt"][sel].cuda(), 1, len(sel))
                torch.cuda.synchronize()
                lg = r["logits"].cpu()
                st = margin_stats(lg, ref)
                kept = top5_set(lg) == top5_set(ref)
                ok = (not y["binds"]) or (kept and st["centred"] <= 0.5 * y["gap"])
                verdict[tag] = verdict.get(tag, True) and ok
                out[f"{name}/q{qi}/{tag}"] = dict(gap_5_6=y["gap"], top5_set_kept=bool(kept), rule_binds=y["binds"], fp8_first_layer=k,
                                                  q8_smooth=smooth, reference_autocast_centred=y["stats"]["centred"], **st)
                line.append(f"q{qi}: |d| {st['max_abs']:.3f} c {st['centred']:.3f} (gap/2 {0.5 * y['gap']:.3f}) rho {st['rho']:.3f} "
                            f"{st['top5']} {'kept' if kept else 'LOST'}")
            print(f"[{name}] {tag:22s} " + "   ".join(line), flush=True)
        del eng
        torch.cuda.empty_cache()
    out["verdict_ranks_with_margin"] = verdict
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
print("verdict (ranks with margin on every binding list):", json.dumps(verdict, sort_keys=True))
print("written", a.json)
