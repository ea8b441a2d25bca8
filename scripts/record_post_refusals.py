#!/usr/bin/env python3
"""Records what the library answers to every refused call of tests/post_refusal_cases.py: {case id: [return code, brt_last_error text]},
packed by post_refusal_cases.pack (the distinct answers once, one line per export).
tests/golden/post_refusals.json was recorded with this on a build of the commit BEFORE the post-pass, upscale and adaptive entry points
were folded onto one skeleton (BRT_LIB_PATH=<that build> python scripts/record_post_refusals.py --out ...); tests/test_post_refusals.py
replays the table on the tree's own build.  Needs one MI355X (a context needs a device); launches nothing.  Refuses to write a table in
which a case came back BRT_OK: such a case is no refusal and does not belong in tests/post_refusal_cases.py."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import post_refusal_cases as prc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "post_refusals.json"))
    args = ap.parse_args()
    got = prc.run_on_gpu()
    accepted = [k for k, (rc, _) in got.items() if rc == 0]
    if accepted:
        sys.exit(f"not refused: {accepted}")
    with open(args.out, "w") as f:
        doc = prc.pack(got)                      # one line per distinct answer, one per export
        f.write('{"answers": [\n' + ",\n".join(json.dumps(a) for a in doc["answers"]) + '],\n"cases": {\n'
                + ",\n".join(f"{json.dumps(e)}: {json.dumps(t)}" for e, t in doc["cases"].items()) + "}}\n")
    print(f"{len(got)} refusals -> {args.out}")


if __name__ == "__main__":
    main()
