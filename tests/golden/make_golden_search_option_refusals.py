"""What the command line and search_options.check() answer to every search option alone and to every pair of them, recorded
from the code as it stood before the side options (moves-left utility, draw average, lower-confidence-bound move choice, c_puct
schedule, policy temperature) moved into a table of their own: tests/test_search_option_refusals_cpu.py replays the
enumeration and compares byte for byte.  No reference code is involved, the recording is this project's own behaviour.

    python tests/golden/make_golden_search_option_refusals.py   ->  tests/golden/search_option_refusals.json
"""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "chinesechess-alphazero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

COMMANDS = ("self", "eval", "reanalyse", "opt")
_RV = ["--record-visits"]
# one legal "on" setting per option group: (values of search_options.VALUES, context flags of check(), command-line words).
# First the 12 rows of OPTIONS, then the five side options, then the two side values that have a command check of their own.
GROUPS = {
    "record_visits": (dict(record_visits=True), {}, _RV),
    "fast_sims": (dict(fast_sims=8), {}, ["--fast-sims", "8"]),
    "forced_playouts": (dict(forced_playouts=2.0, record_visits=True), {}, ["--forced-playouts", "2"] + _RV),
    "record_q": (dict(record_q=True, record_visits=True), {}, ["--record-q"] + _RV),
    "record_surprise": (dict(record_surprise=True, record_visits=True), {}, ["--record-surprise"] + _RV),
    "leaf_mirror": (dict(leaf_mirror=0.5), {}, ["--leaf-mirror", "0.5"]),
    "gumbel": (dict(gumbel=8, record_visits=True), {}, ["--gumbel", "8"] + _RV),
    "gumbel_full": (dict(gumbel=8, gumbel_full=True, record_visits=True), {}, ["--gumbel", "8", "--gumbel-full"] + _RV),
    "eval_cache": (dict(eval_cache=10), {}, ["--eval-cache", "10"]),
    "solver": (dict(solver=True), {}, ["--solver"]),
    "kld_gain": (dict(kld_gain=1e-3), {}, ["--kld-gain", "1e-3"]),
    "smart_pruning": (dict(smart_pruning=True), {}, ["--smart-pruning"]),
    "moves_left": ({}, dict(moves_left=True), ["--moves-left-slope", "0.003"]),
    "draw": ({}, dict(draw=True), ["--draw-score", "0.2"]),
    "lcb": ({}, dict(lcb=True), ["--lcb", "2"]),
    "cpuct": ({}, {}, ["--cpuct-factor", "2"]),
    "policy_temp": ({}, {}, ["--policy-temp", "1.4"]),
    "lcb_min_visits": ({}, {}, ["--lcb-min-visits", "0.3"]),
    "cpuct_base": ({}, {}, ["--cpuct-base", "1000"]),
}


def cases():
    """Every single group and every pair of groups: (name, values, context, words)."""
    for names in itertools.chain(((g,) for g in GROUPS), itertools.combinations(GROUPS, 2)):
        values, context, words = {}, {}, []
        for g in names:
            values.update(GROUPS[g][0])
            context.update(GROUPS[g][1])
            words += [w for w in GROUPS[g][2] if w != "--record-visits" or w not in words]
        yield "+".join(names), values, context, words


def record():
    """{"build_config": {command: {case: "ok" or the SystemExit text}}, "check": {case: {spelling: "ok" or the error text}}}; the
    spellings of check() are key / flag, each also with a script (script=True) beside it."""
    from cchess_alphazero import manager, search_options as so
    parser = manager.create_parser()
    out = dict(build_config={c: {} for c in COMMANDS}, check={})
    for name, values, context, words in cases():
        for cmd in COMMANDS:
            try:
                manager.build_config(parser.parse_args([cmd] + words))
                out["build_config"][cmd][name] = "ok"
            except SystemExit as e:
                out["build_config"][cmd][name] = str(e)
        got = out["check"][name] = {}
        for flags, script in itertools.product((False, True), (False, True)):
            try:
                so.check(dict(values), flags=flags, script=script, **context)
                answer = "ok"
            except so.SearchOptionError as e:
                answer = str(e)
            got[("flag" if flags else "key") + ("+script" if script else "")] = answer
    return out


def main():
    out = record()
    with open(os.path.join(HERE, "search_option_refusals.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    for cmd in COMMANDS:
        answers = out["build_config"][cmd].values()
        print(cmd, len(answers), "cases,", sum(a != "ok" for a in answers), "refused")


if __name__ == "__main__":
    main()
