#!/usr/bin/env python3
"""Merge the resignation-audit histograms that `run.py self --resign-audit` writes (resign_audit_<rank>.json in the
play-data directory) and print the curve: per threshold, how many audited games would have resigned and how many of
those went on to win or draw; then the threshold for a false-positive target.

    python tools/resign_audit.py [--target P] [--min-events N] [--json] FILE [FILE ...]

No device is needed."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "chinesechess-alphazero_amd"))


def merge_files(paths):
    from cchess_alphazero.lib.resign_audit import ResignAudit
    total = None
    for p in paths:
        with open(p) as f:
            a = ResignAudit.from_json(json.load(f))
        total = a if total is None else total.merge(a)
    return total


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("files", nargs="+", metavar="FILE")
    ap.add_argument("--target", type=float, default=0.05, metavar="P", help="false-positive target, 0 < P < 1 (default 0.05)")
    ap.add_argument("--min-events", type=int, default=None, metavar="N",
                    help="games that must have resigned at a threshold before it qualifies (default ceil(5 / P))")
    ap.add_argument("--json", action="store_true", help="print one JSON object instead of the table")
    args = ap.parse_args(argv)
    if not 0.0 < args.target < 1.0:
        raise SystemExit(f"--target {args.target:g}: expected 0 < P < 1")
    try:
        total = merge_files(args.files)
    except (OSError, ValueError, KeyError) as e:
        raise SystemExit(f"resign_audit: {e}")
    t = total.choose_threshold(args.target, args.min_events)
    if args.json:
        print(json.dumps(dict(total.to_json(), target=args.target, chosen=t)))
        return 0
    print(f"{total.games} games audited, {total.skipped} skipped, {len(args.files)} file(s)")
    print(f"{'T':>7s} {'would':>8s} {'fp':>8s} {'fp/would':>9s}")
    rates = total.rates()
    for k, T in enumerate(total.grid):
        if total.would[k] == 0 and (k == 0 or total.would[k - 1] == 0):
            continue                                    # (thresholds nothing ever crossed, but for the last before one did)
        r = f"{rates[k]:9.4f}" if total.would[k] else f"{'-':>9s}"
        print(f"{T:7.2f} {int(total.would[k]):8d} {int(total.fp[k]):8d} {r}")
    print(f"threshold for a false-positive target of {args.target:g}: " + ("none qualifies" if t is None else f"{t:g}"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
