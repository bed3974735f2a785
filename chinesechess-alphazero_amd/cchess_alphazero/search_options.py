"""The search options that travel flag -> config.engine -> engine / player / arena -> Search.set_*, stated once: each one's
values (key, flag, default, range, help), the run.py commands that take it, what it needs, the Search call that switches it
on and its self-play log line -- and the pairs that cannot run beside each other.  No torch, no device.

An option is ON when its first value is truthy (every first default is falsy).  OPTIONS is in the order the options were
added, and a pair of EXCLUDES is (the later option, the earlier one): check() reports in table order, so a refusal reads
`<later> excludes <earlier>: <reason>`.  csrc/xq_search.hip holds the same matrix for the library's setters
(tests/test_gpu_search_options.py pins the two to each other)."""
from collections import namedtuple

INF = float("inf")
EVAL_CACHE_STRIDE = 576      # include/czero.h CZ_EVAL_CACHE_STRIDE

# ok(v, sims) -> bool (None: any value); `expected` completes "<name> <v>: expected ..."; metavar None = a store_true flag
Value = namedtuple("Value", "key flag default metavar ok expected help", defaults=(False, None, None, None, None))
# commands: the run.py commands that accept the option switched on (None: all), command_why: appended to that refusal;
# needs: (key, reason); refused_with: (context key of check(), reason); setter: the Search method, called with the values;
# log: str.format template over all values + sims + eval_cache_mib
Option = namedtuple("Option", "values commands command_why needs refused_with setter log", defaults=(None,) * 6)


def _rate(v, sims):
    return 0.0 <= v <= 1.0              # (false for NaN too)


def _finite(v, sims):
    return 0.0 <= v < INF


OPTIONS = (
    Option([Value("record_visits", "--record-visits",
                  help="(self) play records carry each searched move's root visit counts: [move, value, pi]")]),
    Option([Value("fast_sims", "--fast-sims", 0, "N", lambda v, sims: 0 <= v <= (v if sims is None else sims),
                  "0 <= N <= simulation_num_per_move ({sims})",
                  "(self) playout cap randomization: a ply is a full search with probability --full-rate, otherwise "
                  "a fast one of N simulations without root noise whose row is not trained on (0 = off)"),
            Value("full_rate", "--full-rate", 0.25, "P", _rate, "0 <= P <= 1",
                  "(self, with --fast-sims) probability that a ply is a full search")],
           setter="set_playout_cap",
           log="playout cap: a ply is a full search ({sims} simulations) with probability {full_rate}, otherwise "
               "{fast_sims} simulations without root noise"),
    Option([Value("forced_playouts", "--forced-playouts", 0.0, "K", _finite, "a finite K >= 0",
                  "(self, with --record-visits) forced playouts and policy target pruning: on full plies a "
                  "tried root move is visited at least sqrt(K * prior * visits) times and the recorded "
                  "counts are pruned of the visits that forcing added (0 = off; the paper uses 2)")],
           needs=("record_visits", "forcing without the pruned visit counts only distorts what the trainer sees"),
           setter="set_forced_playouts",
           log="forced playouts k = {forced_playouts} on full plies; the recorded visit counts are pruned (policy target "
               "pruning)"),
    Option([Value("record_q", "--record-q",
                  help="(self, with --record-visits) play records carry each searched ply's root search value: "
                       "[move, value, pi, weight, q], for run.py opt --q-ratio")],
           needs=("record_visits", "the search values ride beside the visit entries"), setter="record_values",
           log="the records carry each searched ply's root search value q (items [move, value, pi, weight, q])"),
    Option([Value("record_surprise", "--record-surprise",
                  help="(self, with --record-visits) play records carry each recorded ply's policy surprise, "
                       "KL(visit counts || network prior): [move, value, pi, weight, q, s], for run.py opt "
                       "--surprise-weight")],
           needs=("record_visits", "the surprises ride beside the visit entries"), setter="record_surprise",
           log="the records carry each recorded ply's policy surprise s (items [move, value, pi, weight, q, s])"),
    Option([Value("leaf_mirror", "--leaf-mirror", 0.0, "P", _rate, "0 <= P <= 1",
                  "(self, eval) random leaf mirror: the search shows every new leaf to the network as its "
                  "left-right mirror image with probability P and reads the policy back through the label "
                  "mirror, so that the network's wing bias averages out of the search (0 = off; 0.5 = a fair "
                  "coin)")],
           setter="set_leaf_mirror",
           log="random leaf mirror: a new leaf is evaluated as its left-right mirror image with probability {leaf_mirror}"),
    Option([Value("gumbel", "--gumbel", 0, "M", lambda v, sims: 0 <= v <= 128, "0 <= M <= 128",
                  "(self, with --record-visits) Gumbel root search: M candidate moves are sampled at the root through "
                  "Gumbel noise, the ply's simulations are spent on them by sequential halving and the survivor is "
                  "played; the recorded pi is softmax(log prior + sigma(completed Q)).  Sound at small --sims "
                  "(0 = off; the paper uses 16)"),
            Value("gumbel_visit", "--gumbel-visit", 50.0, "C", _finite, "a finite C >= 0",
                  "(self, with --gumbel) c_visit of sigma"),
            Value("gumbel_scale", "--gumbel-scale", 1.0, "C", _finite, "a finite C >= 0",
                  "(self, with --gumbel) c_scale of sigma")],
           needs=("record_visits", "the halving counts are not a policy target, the target rides in the visit entries"),
           setter="set_gumbel",
           log="Gumbel root search: {gumbel} candidates, sequential halving over {sims} simulations, c_visit = "
               "{gumbel_visit}, c_scale = {gumbel_scale}; no root noise, no temperature; the recorded pi is "
               "softmax(log prior + sigma(completed Q))"),
    Option([Value("gumbel_full", "--gumbel-full",
                  help="(self, with --gumbel) full Gumbel search: below the root the selection is argmax pi'(a) - "
                       "N(a) / (1 + sum N) instead of PUCT, and the recorded pi completes unvisited moves with v_mix, "
                       "the root's network value mixed with the visited moves' mean")],
           needs=("gumbel", "it completes the Gumbel root search below the root"), setter="set_gumbel_full",
           log="full Gumbel search: below the root argmax pi'(a) - N(a) / (1 + sum N) replaces PUCT, unvisited moves are "
               "completed with v_mix"),
    Option([Value("eval_cache", "--eval-cache", 0, "LOG2", lambda v, sims: v == 0 or 10 <= v <= 24,
                  "0 (off) or 10 <= LOG2 <= 24",
                  "(self) cross-game evaluation cache: a table of 2**LOG2 network results keyed by position "
                  "(576 bytes each), shared by all games and kept across games; a new leaf whose position it "
                  "holds is not evaluated again.  The search stays the same bit for bit (0 = off; 10 <= LOG2 "
                  "<= 24)")],
           commands=("self",),
           command_why=": the arena feeds two networks through one search, and a single game's tree is already its own cache",
           refused_with=("history", "needs the 14-plane input (no use_history): with 28 planes the second block depends on "
                                    "the simulation's path and the game history, so the network input is not a function of "
                                    "the position"),
           setter="set_eval_cache",
           log="evaluation cache: 2^{eval_cache} entries, {eval_cache_mib} MiB, kept across games"),
    Option([Value("solver", "--solver",
                  help="(self, eval) MCTS solver: a position whose every move allows the king's capture is proven lost "
                       "and the move that leads to it wins; proven positions end a simulation without a network "
                       "evaluation, a decided root is not searched further and a won root plays the winning move")],
           commands=("self", "eval"), setter="set_solver",
           log="MCTS solver: forced wins and losses are proven in the tree; a decided root is not searched further, a won "
               "root plays the winning move"),
    Option([Value("kld_gain", "--kld-gain", 0.0, "G", _finite, "a finite G >= 0",
                  "(self) KLD-gain stop: every --kld-interval new root visits the root's visit distribution is "
                  "compared with the previous checkpoint's, and the ply's search ends when the information gained "
                  "per simulation falls below G: quiet positions get short searches (0 = off; lc0's training "
                  "games use values around 1e-5 .. 1e-4)"),
            Value("kld_interval", "--kld-interval", 100, "N", lambda v, sims: v >= 1, "N >= 1",
                  "(self, with --kld-gain) root visits between two checkpoints")],
           commands=("self",), setter="set_kld_gain",
           log="KLD-gain stop: a ply's search ends once its root visit distribution gains less than {kld_gain:g} per "
               "simulation, measured every {kld_interval} root visits"),
    Option([Value("smart_pruning", "--smart-pruning",
                  help="(eval) unreachable-lead stop: a ply whose move is the most visited one ends once that move "
                       "leads the second by more than the simulations not yet started; the move is the one the "
                       "full search would have played from the same tree")],
           commands=("eval",), setter="set_smart_pruning"),
)

_ROOT_RULE = "each defines its own root rule"
_CACHE = "the cache has a kernel instantiation of its own"
EXCLUDES = (("gumbel", "fast_sims", _ROOT_RULE), ("gumbel", "forced_playouts", _ROOT_RULE),
            ("solver", "gumbel", _ROOT_RULE), ("solver", "forced_playouts", _ROOT_RULE), ("solver", "eval_cache", _CACHE),
            ("kld_gain", "gumbel", _ROOT_RULE), ("kld_gain", "solver", _ROOT_RULE), ("kld_gain", "eval_cache", _CACHE),
            ("smart_pruning", "gumbel", _ROOT_RULE), ("smart_pruning", "solver", _ROOT_RULE),
            ("smart_pruning", "eval_cache", _CACHE))

# A script (`run.py reanalyse`, SelfPlayEngine(script=...), Search.set_script) is no value of the table -- it has no flag and no
# config.engine key, the games are its argument -- but it takes part in the exclusions: check(script=True) refuses these
# beside it and asks for what it needs.  The library's setters hold the same list (csrc/xq_search.hip F_SCRIPT;
# tests/test_gpu_reanalyse.py pins the two to each other).  A book and the resignation audit, which are not search options
# either, are refused beside a script by the engine and by the library.
_SCRIPT = "each defines its own root rule, start position or game end"
SCRIPT_EXCLUDES = (("gumbel", _SCRIPT), ("solver", _SCRIPT), ("kld_gain", _SCRIPT), ("smart_pruning", _SCRIPT))
SCRIPT_NEEDS = ("record_visits", "the new targets are the visit entries")

# ---- the side options: what each one excludes, its defaults, its messages and its range check; SIDE below is their table ------
# They are no rows of OPTIONS: the rule "on = first value truthy, default falsy" fits neither the draw average (on with a score
# or with show_wdl) nor T = 1, their flags and help texts are manager._FLAGS' own, and what they need of the network (the
# moves-left output, the win / draw / loss head, logit rows) no table row can say: the layers above ask for that themselves.
#
# The moves-left utility (run.py self / eval --moves-left-slope, engine.moves_left_slope, Search.set_moves_left) needs a network
# with the moves-left output.  The library's setters hold the same list (csrc/xq_search.hip F_ML;
# tests/test_gpu_moves_left_search.py pins the two to each other).
_ML_WORD3 = "the Gumbel search keeps the network value in the node header word that holds the moves-left prediction"
_ML_KERNEL = "each has a kernel instantiation of its own"
MOVES_LEFT_EXCLUDES = (("gumbel", _ML_WORD3), ("solver", _ML_KERNEL), ("kld_gain", _ML_KERNEL), ("smart_pruning", _ML_KERNEL),
                       ("eval_cache", _ML_KERNEL + ", and a cache entry holds no moves-left output"))
MOVES_LEFT_SCRIPT = "reanalysis searches with the recorded games' own rule"
MOVES_LEFT_REFUSAL = ("the moves-left utility (moves_left_slope {slope:g}) needs a model with the moves-left output: train "
                      "one with `run.py opt --moves-left W`")
MOVES_LEFT_DEFAULTS = dict(moves_left_slope=0.0, moves_left_cap=0.0345)
MOVES_LEFT_LOG = ("moves-left utility: slope {moves_left_slope:g} per ply, cap {moves_left_cap:g}; a winning side prefers the "
                  "shorter game, a losing side the longer one")


def check_moves_left(slope, cap, flags=False):
    """Raises SearchOptionError unless slope and cap are finite and >= 0; True when the option is on (slope > 0)."""
    for key, flag, v in (("moves_left_slope", "--moves-left-slope", slope), ("moves_left_cap", "--moves-left-cap", cap)):
        if not _finite(v, None):
            raise SearchOptionError(f"{flag if flags else key} {v}: expected a finite value >= 0")
    return slope > 0.0


# The draw average (run.py self / eval --draw-score, engine.draw_score and engine.show_wdl, Search.set_draw) needs a network with
# the win / draw / loss value head.  The library's setters hold the same list (csrc/xq_search.hip F_DRAW;
# tests/test_gpu_draw_search.py pins the two to each other).
_DRAW_WORD3 = "the Gumbel search keeps the network value in the node header word that holds the leaf's draw probability"
DRAW_EXCLUDES = (("gumbel", _DRAW_WORD3), ("solver", _ML_KERNEL), ("kld_gain", _ML_KERNEL), ("smart_pruning", _ML_KERNEL),
                 ("eval_cache", _ML_KERNEL + ", and a cache entry holds no draw probability"))
DRAW_SCRIPT = "reanalysis searches with the recorded games' own rule"
DRAW_MOVES_LEFT = "an edge's draw record lies where its moves-left record would"
DRAW_REFUSAL = ("the draw average (draw_score {score:g}, show_wdl {show_wdl}) needs a model with the win / draw / loss value "
                "head: train one with `run.py opt --value-head wdl`")
DRAW_DEFAULTS = dict(draw_score=0.0, show_wdl=False)
DRAW_LOG = ("draw average: a draw is worth {draw_score:g} to the side to move at the root; every edge keeps the mean draw "
            "probability of its simulations")


def check_draw(score, show_wdl=False, flags=False):
    """Raises SearchOptionError unless score is finite and in [-1, 1]; True when the average is on (score != 0 or show_wdl)."""
    if not (isinstance(score, (int, float)) and -1.0 <= score <= 1.0):      # (False for NaN)
        raise SearchOptionError(f"{'--draw-score' if flags else 'draw_score'} {score}: expected a finite value in [-1, 1]")
    return score != 0.0 or bool(show_wdl)


# The lower-confidence-bound move choice (run.py self / eval --lcb Z --lcb-min-visits R, engine.lcb and engine.lcb_min_visits,
# Search.set_lcb) needs no special network output.  The library's setters hold the same list (csrc/xq_search.hip F_LCB;
# tests/test_gpu_lcb.py pins the two to each other).
_LCB_KERNEL = "each has a kernel instantiation of its own"
LCB_EXCLUDES = (("gumbel", "the Gumbel search has its own root rule and move choice"),
                ("solver", _LCB_KERNEL + ", and the solver has its own move choice"), ("kld_gain", _LCB_KERNEL),
                ("smart_pruning", "the unreachable-lead stop promises the move of the full search, the most visited one"),
                ("eval_cache", _LCB_KERNEL))
LCB_SCRIPT = "the moves of a reanalysed game are the record's, nothing is chosen"
LCB_MOVES_LEFT = "an edge's value record lies where its moves-left record would"
LCB_DRAW = "an edge's value record lies where its draw record would"
LCB_DEFAULTS = dict(lcb=0.0, lcb_min_visits=0.15)
LCB_LOG = ("lower confidence bound: at temperature 0 the move played has the greatest q - {lcb:g} standard errors among the moves "
           "with at least {lcb_min_visits:g} of the most visited move's visits")


def check_lcb(z, ratio, flags=False):
    """Raises SearchOptionError unless z is finite and >= 0 and ratio is in [0, 1]; True when the option is on (z > 0)."""
    if not (isinstance(z, (int, float)) and _finite(z, None)):
        raise SearchOptionError(f"{'--lcb' if flags else 'lcb'} {z}: expected a finite value >= 0")
    if not (isinstance(ratio, (int, float)) and _rate(ratio, None)):
        raise SearchOptionError(f"{'--lcb-min-visits' if flags else 'lcb_min_visits'} {ratio}: expected a value in [0, 1]")
    return z > 0.0


# The schedule of c_puct (run.py self / eval / reanalyse --cpuct-factor F --cpuct-base B, engine.cpuct_factor and
# engine.cpuct_base, Search.set_cpuct_schedule) and the policy temperature (--policy-temp T, engine.policy_temp,
# Search.set_policy_temperature) are plain parameters of the kernels that run anyway, so they exclude nothing and nothing
# excludes them: check() has no context for them.  The temperature needs logit rows.
CPUCT_DEFAULTS = dict(cpuct_factor=0.0, cpuct_base=19652.0)
CPUCT_LOG = ("c_puct schedule: the exploration constant of a node is c_puct + {cpuct_factor:g} * log((1 + N + {cpuct_base:g}) / "
             "{cpuct_base:g}), N the node's visit count")
POLICY_TEMP_DEFAULTS = dict(policy_temp=1.0)
POLICY_TEMP_LOG = "policy temperature {policy_temp:g}: a node's priors are the softmax of its legal moves' logits / {policy_temp:g}"
POLICY_TEMP_REFUSAL = ("the policy temperature (policy_temp {T:g}) is applied to the legal moves' logits, and {who} hands the "
                       "search probabilities")


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def check_cpuct(factor, base, flags=False):
    """Raises SearchOptionError unless factor is finite and >= 0 and base finite and >= 1; True when the schedule is on
    (factor > 0)."""
    if not (_number(factor) and _finite(factor, None)):
        raise SearchOptionError(f"{'--cpuct-factor' if flags else 'cpuct_factor'} {factor}: expected a finite value >= 0")
    if not (_number(base) and 1.0 <= base < INF):
        raise SearchOptionError(f"{'--cpuct-base' if flags else 'cpuct_base'} {base}: expected a finite value >= 1")
    return factor > 0.0


def check_policy_temp(T, flags=False):
    """Raises SearchOptionError unless 0.1 <= T <= 10; True when the temperature is on (T != 1)."""
    if not (_number(T) and 0.1 <= T <= 10.0):               # (False for NaN)
        raise SearchOptionError(f"{'--policy-temp' if flags else 'policy_temp'} {T}: expected a value in [0.1, 10]")
    return T != 1.0


# The side options in the order they were added, which is the order check() consults them in.
# context: its keyword of check() (None: it takes no part in the exclusions); key, flag: what names it in a message; on: the
# name of its on-flag in resolve_side()'s result; excludes: (key of OPTIONS, reason); script: why it excludes a script;
# earlier: (an earlier row it excludes, reason); values: {key: default}, in the order check and the setter take them;
# check(*values, flags=) -> on, raises for a value out of range; setter, args: the Search method and its arguments, a str being
# the value of that key (setter None: the caller's to switch on); commands: (None: the option is on | the key of a value that
# is off its default, the run.py commands that take it, the sentence that refuses it elsewhere).  The first three let `run.py
# reanalyse` through to check(), whose "excludes a script" gives the reason; --lcb-min-visits alone does not get that far.
Side = namedtuple("Side", "context key flag on excludes script earlier values check setter args commands")
_SEARCHES = ("self", "eval", "reanalyse")
_SELF_EVAL = "{} is an option of `run.py self` and `run.py eval`"
_EVERY_SEARCH = "{} is an option of `run.py self`, `run.py eval` and `run.py reanalyse`"
_ML = Side("moves_left", "moves_left_slope", "--moves-left-slope", "moves_left", MOVES_LEFT_EXCLUDES, MOVES_LEFT_SCRIPT, (),
           MOVES_LEFT_DEFAULTS, check_moves_left, "set_moves_left", ("moves_left_slope", "moves_left_cap"),
           ((None, _SEARCHES, _SELF_EVAL.format("--moves-left-slope")),))
_DRAW = Side("draw", "draw_score", "--draw-score", "draw", DRAW_EXCLUDES, DRAW_SCRIPT, ((_ML, DRAW_MOVES_LEFT),),
             DRAW_DEFAULTS, check_draw, "set_draw", (True, "draw_score"), ((None, _SEARCHES, _SELF_EVAL.format("--draw-score")),))
_LCB = Side("lcb", "lcb", "--lcb", "lcb_on", LCB_EXCLUDES, LCB_SCRIPT, ((_ML, LCB_MOVES_LEFT), (_DRAW, LCB_DRAW)),
            LCB_DEFAULTS, check_lcb, "set_lcb", ("lcb", "lcb_min_visits"),
            ((None, _SEARCHES, _SELF_EVAL.format("--lcb")), ("lcb_min_visits", ("self", "eval"), _SELF_EVAL.format("--lcb-min-visits"))))
SIDE = (_ML, _DRAW, _LCB,
        Side(None, "cpuct_factor", "--cpuct-factor", "cpuct_on", (), None, (), CPUCT_DEFAULTS, check_cpuct,
             "set_cpuct_schedule", ("cpuct_factor", "cpuct_base"),
             ((None, _SEARCHES, _EVERY_SEARCH.format("--cpuct-factor")), ("cpuct_base", _SEARCHES, _EVERY_SEARCH.format("--cpuct-base")))),
        # (set by the caller: the engine after its network is installed, and the player and the arena refuse it)
        Side(None, "policy_temp", "--policy-temp", "policy_temp_on", (), None, (), POLICY_TEMP_DEFAULTS, check_policy_temp,
             None, None, ((None, _SEARCHES, _EVERY_SEARCH.format("--policy-temp")),)))

VALUES ={v.key: v for o in OPTIONS for v in o.values}
DEFAULTS = {k: v.default for k, v in VALUES.items()}


class SearchOptionError(ValueError):
    """A value out of range, an option the command does not take, a missing prerequisite or an excluded pair."""


def flags():
    """(flag, argparse keywords) of every value, for manager._FLAGS."""
    return [(v.flag, dict(action="store_true", help=v.help) if v.metavar is None else
             dict(type=type(v.default), default=v.default, metavar=v.metavar, help=v.help)) for v in VALUES.values()]


def resolve(config, **overrides):
    """{key: value} of the keys named: the override, or for None config.engine's value, or without one the default; each
    in its default's type.  config may lack the engine section."""
    ec = getattr(config, "engine", None)
    return {k: type(DEFAULTS[k])(getattr(ec, k, DEFAULTS[k]) if v is None else v) for k, v in overrides.items()}


def resolve_side(config, **overrides):
    """{key: value} of every value of SIDE, resolved as resolve() does (a key that is not named counts as None), and {on: bool}
    of every row: the attributes an engine, a player and an arena worker keep (moves_left_slope .. policy_temp; moves_left,
    draw, lcb_on, cpuct_on, policy_temp_on).  Raises SearchOptionError for the first value out of range, rows in order."""
    ec = getattr(config, "engine", None)
    side = {}
    for row in SIDE:
        for k, d in row.values.items():
            side[k] = type(d)(getattr(ec, k, d) if overrides.get(k) is None else overrides[k])
        side[row.on] = row.check(*[side[k] for k in row.values])
    return side


def side_of_command(args, cmd):
    """The command line's half of resolve_side(): ({key: value} of every value of SIDE from the parsed arguments, {context: on}
    for check()).  Raises SearchOptionError, per row in order, for a value out of range and then for what `run.py cmd` does not
    take; the messages name the flags."""
    side, context = {}, {}
    for row in SIDE:
        values = {k: type(d)(getattr(args, k, d)) for k, d in row.values.items()}
        on = row.check(*values.values(), flags=True)
        for key, commands, refusal in row.commands:
            if (on if key is None else values[key] != row.values[key]) and cmd not in commands:
                raise SearchOptionError(refusal)
        side.update(values)
        if row.context:
            context[row.context] = on
    return side, context


def apply_side(search, side):
    """Switches on, through their Search methods and in SIDE's order, the side options that are on in resolve_side()'s result
    (all but the policy temperature, which is the caller's)."""
    for row in SIDE:
        if row.setter and side[row.on]:
            getattr(search, row.setter)(*[side[a] if isinstance(a, str) else a for a in row.args])


def check(values, flags=False, cmd=None, sims=None, **context):
    """Raises SearchOptionError for the first violation among the values given (a key that is missing is at its default):
    per option its ranges, the command, its context rule, what it needs, what it excludes; options in table order.
    flags: the messages name --kld-gain where they would name kld_gain.  cmd: the run.py command (None: not checked);
    sims: simulation_num_per_move, the bound of fast_sims (None: not checked); context: history=True for the 28-plane
    input, script=True for scripted games (checked after the table: SCRIPT_NEEDS, SCRIPT_EXCLUDES), and a side option's context
    (moves_left=True, draw=True, lcb=True) for one that is on (checked after that, in SIDE's order: its row's excludes, a script,
    the earlier side options)."""
    def name(key):
        return VALUES[key].flag if flags else key

    def on(key):
        return bool(values.get(key, DEFAULTS[key]))
    for o in OPTIONS:
        key = o.values[0].key
        for v in o.values:
            if v.ok and v.key in values and not v.ok(values[v.key], sims):
                raise SearchOptionError(f"{name(v.key)} {values[v.key]}: expected {v.expected.format(sims=sims)}")
        if not on(key):
            continue
        shown = name(key) if o.values[0].metavar is None else f"{name(key)} {values[key]}"
        if cmd is not None and o.commands and cmd not in o.commands:
            raise SearchOptionError(f"{name(key)} is an option of " + " and ".join(f"`run.py {c}`" for c in o.commands)
                                    + (o.command_why or ""))
        if o.refused_with and context.get(o.refused_with[0]):
            raise SearchOptionError(f"{name(key)} {o.refused_with[1]}")
        if o.needs and not on(o.needs[0]):
            raise SearchOptionError(f"{shown} needs {name(o.needs[0])}: {o.needs[1]}")
        for later, earlier, why in EXCLUDES:
            if later == key and on(earlier):
                raise SearchOptionError(f"{name(later)} excludes {name(earlier)}: {why}")
    if context.get("script"):
        if not on(SCRIPT_NEEDS[0]):
            raise SearchOptionError(f"a script needs {name(SCRIPT_NEEDS[0])}: {SCRIPT_NEEDS[1]}")
        for key, why in SCRIPT_EXCLUDES:
            if on(key):
                raise SearchOptionError(f"a script excludes {name(key)}: {why}")
    for row in SIDE:
        if not (row.context and context.get(row.context)):
            continue
        me = row.flag if flags else row.key
        for key, why in row.excludes:
            if on(key):
                raise SearchOptionError(f"{me} excludes {name(key)}: {why}")
        if context.get("script"):
            raise SearchOptionError(f"{me} excludes a script: {row.script}")
        for earlier, why in row.earlier:
            if context.get(earlier.context):
                raise SearchOptionError(f"{me} excludes {earlier.flag if flags else earlier.key}: {why}")


def apply(search, values, skip=()):
    """Switches on, through their Search methods and in table order, the options that are on among the values given."""
    for o in OPTIONS:
        if o.setter and o.values[0].key not in skip and values.get(o.values[0].key):
            getattr(search, o.setter)(*[values[v.key] for v in o.values])


def describe(values, sims):
    """The self-play log line of every option that is on, in table order."""
    mib = (EVAL_CACHE_STRIDE << values.get("eval_cache", 0)) >> 20
    return [o.log.format(sims=sims, eval_cache_mib=mib, **values) for o in OPTIONS if o.log and values.get(o.values[0].key)]
