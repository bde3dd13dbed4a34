"""Records tests/golden/staged_ws_bytes.json: the workspace (zkp_debug_ws_bytes) after each call of tests/staged_ws_cases.py on a fresh test-hook
context, with the commit it was recorded at.  Run it on the commit whose layouts are the reference -- tests/test_gpu_staged_ws_bytes.py then holds
later commits to them -- on a machine with the GPU, after the libraries are built:

    python tools/record_staged_ws_bytes.py [--out FILE] [--commit HASH]

--commit names the commit where the tree is not a git checkout (default: git rev-parse HEAD)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "staged_ws_bytes.json"))
    ap.add_argument("--commit", default=None)
    args = ap.parse_args()
    commit = args.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    from tests.staged_ws_cases import CASES
    from zkp_amd.engine import Engine
    ws = {}
    for name, call in CASES.items():
        eng = Engine(0, test_hooks=True)
        try:
            call(eng)
            ws[name] = eng.debug_ws_bytes()
        finally:
            eng.close()
        print("%-44s %d" % (name, ws[name]), flush=True)
    with open(args.out, "w") as f:
        json.dump({"recorded_at_commit": commit, "ws_bytes": ws}, f, indent=1)
        f.write("\n")
    print("wrote %s (%d cases, commit %s)" % (args.out, len(ws), commit))


if __name__ == "__main__":
    main()
