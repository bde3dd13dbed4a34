#!/usr/bin/env python3
"""Constant-time evidence for zkp_transcripts_witness_rng (zkp_mi355x.h (7)), by the recipe of tools/ct_check_scalar_scan.py: the 171 start
states of tests/transcript_ops_cases.py (every STROBE position 0..165, so the lanes of a wavefront stand at different positions) run per
witness shape and output mode over three very different classes of witness and entropy bytes -- all 0x00, all 0xff, random -- with
rocprofv3 counting the executed instructions and the LDS bank conflicts of every dispatch: counters only, no tracing in the same run; the
instruction counters and the LDS counters in two runs of their own.  Positions, shapes, counts and the label are equal across the classes.
Equal counters across the classes: no branch was taken or skipped, no load or store issued and no LDS cycle spent because of a witness, an
entropy or a state byte (the keyed state differs from class to class from the first KEY on).

    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_LDS SQ_WAVES \\
              --output-format csv -d OUT_A -o tr -- python tools/ct_check_transcript_rng.py
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_LDS_ADDR_CONFLICT \\
              --output-format csv -d OUT_B -o tr -- python tools/ct_check_transcript_rng.py
    python tools/ct_check_transcript_rng.py --summarise OUT_A/.../tr_counter_collection.csv OUT_B/.../tr_counter_collection.csv
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SHAPES = [(1, 32), (11, 32), (2, 333)]
MODES = [(0, 2), (0, 11), (1, 167)]          # (ZKP_RNG_SCALARS, count), (ZKP_RNG_BYTES, count)
CLASSES = ["0x00", "0xff", "random"]
WATCHED = ("k_strobe_witness_rng",)


def secret_bytes(kind, rng, shape):
    if kind == "random":
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    return np.full(shape, 0 if kind == "0x00" else 0xff, np.uint8)


def run():
    from tests.transcript_ops_cases import start_states
    from zkp_amd.engine import Engine
    eng = Engine(0)
    rng = np.random.default_rng(9)
    S = start_states()
    for m, wlen in SHAPES:                               # per shape and mode one call per class, in this order
        for mode, count in MODES:
            for kind in CLASSES:
                eng.transcripts_witness_rng(S, b"", secret_bytes(kind, rng, (len(S), m, wlen)), secret_bytes(kind, rng, (len(S), 32)), mode, count)
    eng.close()


def summarise(paths):
    import collections
    import csv
    rows = [r for p in paths for r in csv.DictReader(open(p))]
    per = collections.defaultdict(lambda: collections.defaultdict(list))      # kernel -> counter -> values in dispatch order
    for r in sorted(rows, key=lambda r: int(r["Dispatch_Id"])):
        per[r["Kernel_Name"].split("(")[0].replace("void ", "").replace("zkp::", "")][r["Counter_Name"]].append(float(r["Counter_Value"]))
    print("# zkp_transcripts_witness_rng over 171 transcripts at every position 0..165; witness shapes (m, wlen) %s x (mode, count) %s; per shape and mode"
          " one call per class of witness and entropy bytes (%s): the dispatches are listed shape by shape, mode by mode, class by class"
          % (SHAPES, MODES, ", ".join(CLASSES)))
    ok = True
    seen = set()
    dispatches = 0
    for k in sorted(per):                                # (one instantiation per output mode: k_strobe_witness_rng<0u> the scalars, <1u> the bytes)
        watched = [w for w in WATCHED if k.startswith(w)]
        if not watched:
            continue
        seen.update(watched)
        dispatches += len(next(iter(per[k].values())))
        for c, v in sorted(per[k].items()):
            same = len(v) % len(CLASSES) == 0 and all(v[i] == v[i - i % len(CLASSES)] for i in range(len(v)))
            ok &= same
            print("%-28s %-22s %s  %s" % (k[:28], c, "IDENTICAL" if same else "DIFFERENT", " ".join("%.0f" % x for x in v)))
    ok &= seen == set(WATCHED) and dispatches == len(SHAPES) * len(MODES) * len(CLASSES)
    print("# verdict:", "every counter of the RNG kernel identical across the classes of witness and entropy bytes" if ok else "counters differ or the kernel is missing")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2:])
    else:
        run()
