"""Command line of ``run.py`` -- same sub-commands and flags as the reference's cchess_alphazero/manager.py.
``self`` (the hot path), ``opt`` (the trainer, worker/optimize.py) and ``eval`` (the arena) are served by
the MI355X engine; the other sub-commands of the reference (play, sl, ob) are outside the scope table and say
so."""
import argparse
from logging import getLogger

from cchess_alphazero.config import Config
from cchess_alphazero.lib.logger import setup_logger

logger = getLogger(__name__)

COMMANDS = ('self', 'opt', 'eval', 'play', 'sl', 'ob')
PIECE_STYLES = ('WOOD', 'POLISH', 'DELICATE')
BOARD_STYLES = ('CANVAS', 'DROPS', 'GREEN', 'QIANHONG', 'SHEET', 'SKELETON', 'WHITE', 'WOOD')
RANDOMNESS = ('none', 'small', 'medium', 'large')

# (flag, kwargs) -- the reference's options first (manager.py:16-33), then the engine's own
_FLAGS = [
    ("--new", dict(action="store_true", help="run from new best model")),
    ("--type", dict(default="mini", help="configuration: mini / normal / distribute")),
    ("--total-step", dict(type=int, help="TrainerConfig.start_total_steps")),
    ("--ai-move-first", dict(action="store_true", help="(play) the AI moves first")),
    ("--cli", dict(action="store_true", help="(play) command-line board")),
    ("--gpu", dict(default="0", help="comma separated device list; one engine process per device")),
    ("--onegreen", dict(action="store_true", help="(sl) onegreen data")),
    ("--skip", dict(default=0, type=int, help="(sl) skip games")),
    ("--ucci", dict(action="store_true", help="(self) play against a UCCI engine")),
    ("--piece-style", dict(choices=PIECE_STYLES, default="WOOD")),
    ("--bg-style", dict(choices=BOARD_STYLES, default="WOOD")),
    ("--random", dict(choices=RANDOMNESS, default="none")),
    ("--distributed", dict(action="store_true", help="upload / download through the cczero server")),
    ("--elo", dict(action="store_true", help="(eval) server-driven Elo evaluation")),
    ("--games-per-gpu", dict(type=int, help="engine: concurrent games per GPU")),
    ("--net-dtype", dict(choices=["float32", "bfloat16", "float16"], help="engine: network precision")),
    ("--max-rounds", dict(type=int, help="engine: stop after this many lock-step rounds (default: never)")),
    ("--max-games", dict(type=int, help="engine: stop after this many finished games (default: never)")),
    ("--record-visits", dict(action="store_true",
                             help="(self) play records carry each searched move's root visit counts: [move, value, pi]")),
    ("--book", dict(metavar="FILE", help="(self, eval) start-position book: one state string or FEN per line; self-play game "
                                         "i starts from position i mod n, the arena plays each position once per colour")),
    ("--book-rate", dict(type=float, default=1.0, metavar="P",
                         help="(self) a game starts from the book with probability P, otherwise from the opening position")),
    ("--fast-sims", dict(type=int, default=0, metavar="N",
                         help="(self) playout cap randomization: a ply is a full search with probability --full-rate, otherwise "
                              "a fast one of N simulations without root noise whose row is not trained on (0 = off)")),
    ("--full-rate", dict(type=float, default=0.25, metavar="P",
                         help="(self, with --fast-sims) probability that a ply is a full search")),
    ("--forced-playouts", dict(type=float, default=0.0, metavar="K",
                               help="(self, with --record-visits) forced playouts and policy target pruning: on full plies a "
                                    "tried root move is visited at least sqrt(K * prior * visits) times and the recorded "
                                    "counts are pruned of the visits that forcing added (0 = off; the paper uses 2)")),
    ("--record-q", dict(action="store_true",
                        help="(self, with --record-visits) play records carry each searched ply's root search value: "
                             "[move, value, pi, weight, q], for run.py opt --q-ratio")),
    ("--q-ratio", dict(type=float, default=0.0, metavar="L",
                       help="(opt) value target z + L (q - z): the game result mixed with the records' root search values "
                            "where they have one (0 <= L <= 1; 0 = the game result alone, the reference)")),
    ("--record-surprise", dict(action="store_true",
                               help="(self, with --record-visits) play records carry each recorded ply's policy surprise, "
                                    "KL(visit counts || network prior): [move, value, pi, weight, q, s], for run.py opt "
                                    "--surprise-weight")),
    ("--surprise-weight", dict(type=float, default=0.0, metavar="A",
                               help="(opt) policy surprise weighting: within a game, the share A of the training weight goes "
                                    "to the rows in proportion to their recorded surprise (0 <= A <= 1; 0 = uniform, the "
                                    "reference; KataGo uses 0.5)")),
    ("--leaf-mirror", dict(type=float, default=0.0, metavar="P",
                           help="(self, eval) random leaf mirror: the search shows every new leaf to the network as its "
                                "left-right mirror image with probability P and reads the policy back through the label "
                                "mirror, so that the network's wing bias averages out of the search (0 = off; 0.5 = a fair "
                                "coin)")),
    ("--gumbel", dict(type=int, default=0, metavar="M",
                      help="(self, with --record-visits) Gumbel root search: M candidate moves are sampled at the root through "
                           "Gumbel noise, the ply's simulations are spent on them by sequential halving and the survivor is "
                           "played; the recorded pi is softmax(log prior + sigma(completed Q)).  Sound at small --sims "
                           "(0 = off; the paper uses 16)")),
    ("--gumbel-visit", dict(type=float, default=50.0, metavar="C", help="(self, with --gumbel) c_visit of sigma")),
    ("--gumbel-scale", dict(type=float, default=1.0, metavar="C", help="(self, with --gumbel) c_scale of sigma")),
    ("--gumbel-full", dict(action="store_true",
                           help="(self, with --gumbel) full Gumbel search: below the root the selection is argmax pi'(a) - "
                                "N(a) / (1 + sum N) instead of PUCT, and the recorded pi completes unvisited moves with v_mix, "
                                "the root's network value mixed with the visited moves' mean")),
    ("--eval-cache", dict(type=int, default=0, metavar="LOG2",
                          help="(self) cross-game evaluation cache: a table of 2**LOG2 network results keyed by position "
                               "(576 bytes each), shared by all games and kept across games; a new leaf whose position it "
                               "holds is not evaluated again.  The search stays the same bit for bit (0 = off; 10 <= LOG2 "
                               "<= 24)")),
    ("--solver", dict(action="store_true",
                      help="(self, eval) MCTS solver: a position whose every move allows the king's capture is proven lost "
                           "and the move that leads to it wins; proven positions end a simulation without a network "
                           "evaluation, a decided root is not searched further and a won root plays the winning move")),
    ("--kld-gain", dict(type=float, default=0.0, metavar="G",
                        help="(self) KLD-gain stop: every --kld-interval new root visits the root's visit distribution is "
                             "compared with the previous checkpoint's, and the ply's search ends when the information gained "
                             "per simulation falls below G: quiet positions get short searches (0 = off; lc0's training "
                             "games use values around 1e-5 .. 1e-4)")),
    ("--kld-interval", dict(type=int, default=100, metavar="N",
                            help="(self, with --kld-gain) root visits between two checkpoints")),
    ("--smart-pruning", dict(action="store_true",
                             help="(eval) unreachable-lead stop: a ply whose move is the most visited one ends once that move "
                                  "leads the second by more than the simulations not yet started; the move is the one the "
                                  "full search would have played from the same tree")),
    ("--sims", dict(type=int, default=None, metavar="N",
                    help="(self) simulations per move (default: the configuration's simulation_num_per_move)")),
    ("--policy-targets", dict(choices=["played", "visits"], default="played",
                              help="(opt) policy targets: the played move's one-hot (the reference) or the records' root "
                                   "visit counts")),
    ("--augment", dict(choices=["none", "mirror"], default="none",
                       help="(opt) mirror: every training row of every epoch is the left-right mirrored position with "
                            "probability 1/2 (planes and policy targets, in the trainer's kernels)")),
]


def create_parser():
    parser = argparse.ArgumentParser(description="Xiangqi AlphaZero self-play on MI355X")
    parser.add_argument("cmd", choices=COMMANDS, help="what to do")
    for flag, kw in _FLAGS:
        parser.add_argument(flag, **kw)
    return parser


def build_config(args):
    config = Config(config_type=args.type)
    opts, engine = config.opts, config.engine
    opts.new = args.new
    opts.piece_style, opts.bg_style = args.piece_style, args.bg_style
    opts.device_list = args.gpu
    n_dev = len(args.gpu.split(','))
    if n_dev > 1:                                           # reference manager.py:66-70
        opts.use_multiple_gpus, opts.gpu_num = True, n_dev
    config.internet.distributed = args.distributed
    if args.total_step is not None:
        config.trainer.start_total_steps = args.total_step
    if args.games_per_gpu:
        engine.games_per_gpu = args.games_per_gpu
    if args.net_dtype:
        engine.net_dtype = args.net_dtype
    engine.max_rounds, engine.max_games = args.max_rounds, args.max_games
    if args.record_visits:
        engine.record_visits = True
    if not 0.0 <= args.book_rate <= 1.0:
        raise SystemExit(f"--book-rate {args.book_rate}: expected 0 <= P <= 1")
    engine.book_path, engine.book_rate = args.book, args.book_rate
    if args.sims is not None:
        if args.cmd != "self":
            raise SystemExit("--sims is an option of `run.py self`")
        if args.sims < 1:
            raise SystemExit(f"--sims {args.sims}: expected N >= 1")
        config.play.simulation_num_per_move = args.sims
    if not 0 <= args.fast_sims <= config.play.simulation_num_per_move:
        raise SystemExit(f"--fast-sims {args.fast_sims}: expected 0 <= N <= simulation_num_per_move "
                         f"({config.play.simulation_num_per_move})")
    if not 0.0 <= args.full_rate <= 1.0:
        raise SystemExit(f"--full-rate {args.full_rate}: expected 0 <= P <= 1")
    engine.fast_sims, engine.full_rate = args.fast_sims, args.full_rate
    if not 0.0 <= args.forced_playouts < float("inf"):
        raise SystemExit(f"--forced-playouts {args.forced_playouts}: expected a finite K >= 0")
    if args.forced_playouts and not engine.record_visits:
        raise SystemExit(f"--forced-playouts {args.forced_playouts} needs --record-visits: forcing without the pruned "
                         "visit counts only distorts what the trainer sees")
    engine.forced_playouts = args.forced_playouts
    if args.record_q and not engine.record_visits:
        raise SystemExit("--record-q needs --record-visits: the search values ride beside the visit entries")
    if args.record_q:
        engine.record_q = True
    if not 0.0 <= args.q_ratio <= 1.0:
        raise SystemExit(f"--q-ratio {args.q_ratio}: expected 0 <= L <= 1")
    config.trainer.q_ratio = args.q_ratio
    if args.record_surprise and not engine.record_visits:
        raise SystemExit("--record-surprise needs --record-visits: the surprises ride beside the visit entries")
    if args.record_surprise:
        engine.record_surprise = True
    if not 0.0 <= args.surprise_weight <= 1.0:
        raise SystemExit(f"--surprise-weight {args.surprise_weight}: expected 0 <= A <= 1")
    config.trainer.surprise_weight = args.surprise_weight
    if not 0.0 <= args.leaf_mirror <= 1.0:                  # (false for NaN too)
        raise SystemExit(f"--leaf-mirror {args.leaf_mirror}: expected 0 <= P <= 1")
    engine.leaf_mirror = args.leaf_mirror
    if not 0 <= args.gumbel <= 128:
        raise SystemExit(f"--gumbel {args.gumbel}: expected 0 <= M <= 128")
    for name in ("gumbel_visit", "gumbel_scale"):
        if not 0.0 <= getattr(args, name) < float("inf"):
            raise SystemExit(f"--{name.replace('_', '-')} {getattr(args, name)}: expected a finite C >= 0")
    if args.gumbel and not engine.record_visits:
        raise SystemExit(f"--gumbel {args.gumbel} needs --record-visits: the halving counts are not a policy target, the "
                         "target rides in the visit entries")
    if args.gumbel and args.fast_sims:
        raise SystemExit("--gumbel excludes --fast-sims: each defines its own root rule")
    if args.gumbel and args.forced_playouts:
        raise SystemExit("--gumbel excludes --forced-playouts: each defines its own root rule")
    if args.gumbel_full and not args.gumbel:
        raise SystemExit("--gumbel-full needs --gumbel M: it completes the Gumbel root search below the root")
    engine.gumbel, engine.gumbel_visit, engine.gumbel_scale = args.gumbel, args.gumbel_visit, args.gumbel_scale
    engine.gumbel_full = bool(args.gumbel_full)
    if args.eval_cache:
        if args.cmd != "self":
            raise SystemExit("--eval-cache is an option of `run.py self`: the arena feeds two networks through one search, "
                             "and a single game's tree is already its own cache")
        if not 10 <= args.eval_cache <= 24:
            raise SystemExit(f"--eval-cache {args.eval_cache}: expected 0 (off) or 10 <= LOG2 <= 24")
        if getattr(config.model, "input_depth", 14) == 28:
            raise SystemExit("--eval-cache needs the 14-plane input: with 28 planes the second block depends on the "
                             "simulation's path and the game history, so the network input is not a function of the position")
    engine.eval_cache = args.eval_cache
    if args.solver and args.cmd not in ("self", "eval"):
        raise SystemExit("--solver is an option of `run.py self` and `run.py eval`")
    if args.solver and args.gumbel:
        raise SystemExit("--solver excludes --gumbel: each defines its own root rule")
    if args.solver and args.forced_playouts:
        raise SystemExit("--solver excludes --forced-playouts: each defines its own root rule")
    if args.solver and args.eval_cache:
        raise SystemExit("--solver excludes --eval-cache: the cache has a kernel instantiation of its own")
    engine.solver = bool(args.solver)
    if not 0.0 <= args.kld_gain < float("inf"):             # (false for NaN too)
        raise SystemExit(f"--kld-gain {args.kld_gain}: expected a finite G >= 0")
    if args.kld_interval < 1:
        raise SystemExit(f"--kld-interval {args.kld_interval}: expected N >= 1")
    if args.kld_gain and args.cmd != "self":
        raise SystemExit("--kld-gain is an option of `run.py self`")
    if args.smart_pruning and args.cmd != "eval":
        raise SystemExit("--smart-pruning is an option of `run.py eval`")
    for flag, on in (("--kld-gain", bool(args.kld_gain)), ("--smart-pruning", bool(args.smart_pruning))):
        if on and args.gumbel:
            raise SystemExit(f"{flag} excludes --gumbel: each defines its own root rule")
        if on and args.solver:
            raise SystemExit(f"{flag} excludes --solver: each defines its own root rule")
        if on and args.eval_cache:
            raise SystemExit(f"{flag} excludes --eval-cache: the cache has a kernel instantiation of its own")
    engine.kld_gain, engine.kld_interval = args.kld_gain, args.kld_interval
    engine.smart_pruning = bool(args.smart_pruning)
    config.trainer.policy_targets = args.policy_targets
    config.trainer.augment = args.augment
    return config


def start():
    args = create_parser().parse_args()
    config = build_config(args)
    config.resource.create_directories()
    rc = config.resource
    setup_logger({'self': rc.play_log_path, 'eval': rc.eval_log_path, 'opt': rc.opt_log_path}.get(args.cmd, rc.main_log_path))
    logger.info('Config type: %s' % (args.type))
    if args.cmd == 'self':
        if args.ucci:
            raise SystemExit("self-play against an external UCCI engine is outside the MI355X hot path")
        from cchess_alphazero.worker import self_play
        return self_play.start(config)
    if args.cmd == 'eval':                                  # reference manager.py:94-103
        if args.elo:
            raise SystemExit("the server-driven Elo evaluator needs cczero.org (no network): outside the hot path")
        config.eval.update_play_config(config.play)
        # (config.opts.evaluate stays False here, as in the reference: only its Elo evaluator sets it,
        #  compute_elo.py:88 -- so a repeated position is still played at tau = 0.5, player.py:460-461)
        from cchess_alphazero.worker import evaluator
        return evaluator.start(config)
    if args.cmd == 'opt':                                   # reference manager.py:85-87
        from cchess_alphazero.worker import optimize
        return optimize.start(config)
    raise SystemExit(f"`run.py {args.cmd}` is not part of the MI355X self-play hot path (SURVEY 8): use the reference "
                     f"implementation for it; the play records written by `run.py self` are in the reference's format")
