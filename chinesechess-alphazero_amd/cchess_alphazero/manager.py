"""Command line of ``run.py`` -- same sub-commands and flags as the reference's cchess_alphazero/manager.py.
``self`` (the hot path), ``opt`` (the trainer, worker/optimize.py), ``eval`` (the arena) and ``reanalyse``
(stored games searched again with the best model, worker/reanalyse.py; the reference has no such command) are served by
the MI355X engine; the other sub-commands of the reference (play, sl, ob) are outside the scope table and say
so."""
import argparse
from logging import getLogger

from cchess_alphazero import search_options
from cchess_alphazero.config import Config
from cchess_alphazero.lib.logger import setup_logger

logger = getLogger(__name__)

COMMANDS = ('self', 'opt', 'eval', 'reanalyse', 'play', 'sl', 'ob')
PIECE_STYLES = ('WOOD', 'POLISH', 'DELICATE')
BOARD_STYLES = ('CANVAS', 'DROPS', 'GREEN', 'QIANHONG', 'SHEET', 'SKELETON', 'WHITE', 'WOOD')
RANDOMNESS = ('none', 'small', 'medium', 'large')

# (flag, kwargs) -- the reference's options first (manager.py:16-33), then the engine's own; the search options' flags come
# from their table (search_options.py)
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
    ("--book", dict(metavar="FILE", help="(self, eval) start-position book: one state string or FEN per line; self-play game "
                                         "i starts from position i mod n, the arena plays each position once per colour")),
    ("--book-rate", dict(type=float, default=1.0, metavar="P",
                         help="(self) a game starts from the book with probability P, otherwise from the opening position")),
    ("--q-ratio", dict(type=float, default=0.0, metavar="L",
                       help="(opt) value target z + L (q - z): the game result mixed with the records' root search values "
                            "where they have one (0 <= L <= 1; 0 = the game result alone, the reference)")),
    ("--surprise-weight", dict(type=float, default=0.0, metavar="A",
                               help="(opt) policy surprise weighting: within a game, the share A of the training weight goes "
                                    "to the rows in proportion to their recorded surprise (0 <= A <= 1; 0 = uniform, the "
                                    "reference; KataGo uses 0.5)")),
    ("--records", dict(metavar="DIR", help="(reanalyse) the record files to walk again (default: data_dir/trained, where "
                                           "`run.py opt` moves what it has trained on); a finished file moves to DIR/reanalysed")),
    ("--out", dict(metavar="DIR", help="(reanalyse) where the new records go (default: the play-data directory, under names "
                                       "`run.py opt` picks up)")),
    ("--reanalyse-plies", dict(type=int, default=None, metavar="N",
                               help="(reanalyse) plies of stored games handed to the device at once: a batch is all games of "
                                    "as many files as fit (default 200000)")),
    ("--sims", dict(type=int, default=None, metavar="N",
                    help="(self, reanalyse) simulations per move (default: the configuration's simulation_num_per_move)")),
    ("--policy-targets", dict(choices=["played", "visits"], default="played",
                              help="(opt) policy targets: the played move's one-hot (the reference) or the records' root "
                                   "visit counts")),
    ("--augment", dict(choices=["none", "mirror"], default="none",
                       help="(opt) mirror: every training row of every epoch is the left-right mirrored position with "
                            "probability 1/2 (planes and policy targets, in the trainer's kernels)")),
    ("--policy-mask", dict(choices=["none", "legal"], default="none",
                           help="(opt) legal: the policy softmax, its loss and its gradient run over each position's legal "
                                "moves, the distribution the search reads, instead of all 2086 labels (the mask is generated "
                                "in the loss kernel from the window's boards)")),
    ("--moves-left", dict(type=float, default=0.0, metavar="W",
                          help="(opt) train the moves-left output (one more Dense(1) on the value head's hidden layer, "
                               "predicting the plies until the game ends) with the loss weight W (finite, >= 0; 0 = off); a "
                               "new model (--new, or no best model yet) is built with the output, a best model without it "
                               "is refused")),
    ("--moves-left-slope", dict(type=float, default=0.0, metavar="S",
                                help="(self, eval) moves-left utility: the search adds -+ clamp(S * (an edge's mean plies to the "
                                     "end - the node's), cap) * f(|q|) to an edge's score, so that a winning side prefers the "
                                     "shorter game and a losing side the longer one; needs a model with the moves-left output "
                                     "(`run.py opt --moves-left`) (finite, >= 0; 0 = off; lc0 uses 0.0027)")),
    ("--moves-left-cap", dict(type=float, default=0.0345, metavar="C",
                              help="(self, eval, with --moves-left-slope) the bound of the utility before f(|q|) (finite, >= 0)")),
    ("--draw-score", dict(type=float, default=0.0, metavar="S",
                          help="(self, eval) draw score: the search keeps a mean draw probability per edge and adds +-S * that "
                               "mean to an edge's score, S being what a draw is worth to the side to move at the root (so S < 0 "
                               "avoids draws and S > 0 seeks them); needs a model with the win / draw / loss value head "
                               "(`run.py opt --value-head wdl`) (finite, in [-1, 1]; 0 = off)")),
    ("--lcb", dict(type=float, default=0.0, metavar="Z",
                   help="(self, eval) lower confidence bound: where the temperature is 0 the move played is the one with the "
                        "greatest q - Z standard errors of its backed-up values instead of the most visited one; the tree keeps "
                        "a second moment per edge; works with every model (finite, >= 0; 0 = off; KataGo and lc0 use values "
                        "around 2)")),
    ("--lcb-min-visits", dict(type=float, default=0.15, metavar="R",
                              help="(self, eval, with --lcb) a move takes part with at least R times the most visited move's "
                                   "visits (in [0, 1])")),
    ("--cpuct-factor", dict(type=float, default=0.0, metavar="F",
                            help="(self, eval, reanalyse) c_puct schedule: the exploration constant of a node grows with its "
                                 "visit count N, c_puct + F * log((1 + N + B) / B), as in AlphaZero's paper (finite, >= 0; 0 = off: "
                                 "the constant c_puct; lc0 uses 3.894 with --cpuct-base 38739)")),
    ("--cpuct-base", dict(type=float, default=19652.0, metavar="B",
                          help="(self, eval, reanalyse, with --cpuct-factor) the base B of the schedule (finite, >= 1)")),
    ("--policy-temp", dict(type=float, default=1.0, metavar="T",
                           help="(self, eval, reanalyse) policy temperature: a node's priors are the softmax of its legal moves' "
                                "logits divided by T, so T > 1 flattens a policy that training on visit counts has sharpened "
                                "(0.1 <= T <= 10; 1 = off; lc0 uses 1.4 .. 1.6); needs a network that hands over logits")),
    ("--value-head", dict(choices=["scalar", "wdl"], default=None,
                          help="(opt) the value head of a new model (--new, or no best model yet): scalar = Dense(1) + tanh, "
                               "the reference; wdl = Dense(3) + softmax over win / draw / loss, trained by cross-entropy "
                               "(default: what the best model has, scalar for a new one); refused when the best model has "
                               "the other head")),
    ("--resign-audit", dict(action="store_true",
                            help="(self) audit resignation on the games that play on without it: per threshold of a grid, how "
                                 "many would have resigned and how many of those went on to win or draw (needs "
                                 "--record-visits)")),
    ("--resign-fp-target", dict(type=float, default=0.0, metavar="P",
                                help="(self) adapt the resign threshold to the largest one whose false-positive share stays "
                                     "within P (0 < P < 1; 0 = keep the configuration's; needs --resign-audit)")),
] + search_options.flags()


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
    if not 0.0 <= args.book_rate <= 1.0:
        raise SystemExit(f"--book-rate {args.book_rate}: expected 0 <= P <= 1")
    engine.book_path, engine.book_rate = args.book, args.book_rate
    if args.sims is not None:
        if args.cmd not in ("self", "reanalyse"):
            raise SystemExit("--sims is an option of `run.py self` and `run.py reanalyse`")
        if args.sims < 1:
            raise SystemExit(f"--sims {args.sims}: expected N >= 1")
        config.play.simulation_num_per_move = args.sims
    # the search options: ranges, commands, prerequisites and exclusions are their table's (search_options.py)
    values = {k: getattr(args, k) for k in search_options.VALUES}
    reanalyse = args.cmd == "reanalyse"
    if reanalyse:                                           # the new targets are the visit entries
        values["record_visits"] = True
        if args.book:
            raise SystemExit("--book is not an option of `run.py reanalyse`: every stored game has its own start position")
    elif args.records or args.out or args.reanalyse_plies is not None:
        raise SystemExit("--records, --out and --reanalyse-plies are options of `run.py reanalyse`")
    if args.reanalyse_plies is not None and args.reanalyse_plies < 1:
        raise SystemExit(f"--reanalyse-plies {args.reanalyse_plies}: expected N >= 1")
    engine.reanalyse_records, engine.reanalyse_out, engine.reanalyse_plies = args.records, args.out, args.reanalyse_plies
    try:
        side, side_on = search_options.side_of_command(args, args.cmd)     # moves_left_slope .. policy_temp (SIDE)
        search_options.check(values, flags=True, cmd=args.cmd, sims=config.play.simulation_num_per_move,
                             history=getattr(config.model, "input_depth", 14) == 28, script=reanalyse, **side_on)
    except search_options.SearchOptionError as e:
        raise SystemExit(str(e))
    vars(engine).update(values, **side)
    # the resignation audit: game-loop options, not search options; their one check is the library's
    from cchess_alphazero.lib.resign_audit import check_options
    try:
        check_options(args.resign_audit, args.resign_fp_target, values["record_visits"], cmd=args.cmd)
    except ValueError as e:
        raise SystemExit(str(e))
    engine.resign_audit, engine.resign_fp_target = bool(args.resign_audit), float(args.resign_fp_target)
    if not 0.0 <= args.q_ratio <= 1.0:
        raise SystemExit(f"--q-ratio {args.q_ratio}: expected 0 <= L <= 1")
    config.trainer.q_ratio = args.q_ratio
    if not 0.0 <= args.surprise_weight <= 1.0:
        raise SystemExit(f"--surprise-weight {args.surprise_weight}: expected 0 <= A <= 1")
    config.trainer.surprise_weight = args.surprise_weight
    if args.value_head is not None and args.cmd != "opt":
        raise SystemExit("--value-head is an option of `run.py opt`")
    if args.value_head == "wdl" and args.q_ratio > 0.0:
        raise SystemExit(f"--q-ratio {args.q_ratio:g} with --value-head wdl: a scalar q does not determine a distribution "
                         "over win / draw / loss")
    config.trainer.value_head = args.value_head
    if not 0.0 <= args.moves_left < float("inf"):           # (NaN fails both comparisons)
        raise SystemExit(f"--moves-left {args.moves_left}: expected a finite W >= 0")
    if args.moves_left and args.cmd != "opt":
        raise SystemExit("--moves-left is an option of `run.py opt`")
    config.trainer.moves_left = args.moves_left
    if args.policy_mask != "none" and args.cmd != "opt":
        raise SystemExit("--policy-mask is an option of `run.py opt`")
    config.trainer.policy_mask = args.policy_mask
    config.trainer.policy_targets = args.policy_targets
    config.trainer.augment = args.augment
    return config


def start():
    args = create_parser().parse_args()
    config = build_config(args)
    config.resource.create_directories()
    rc = config.resource
    setup_logger({'self': rc.play_log_path, 'reanalyse': rc.play_log_path, 'eval': rc.eval_log_path, 'opt': rc.opt_log_path}.get(args.cmd, rc.main_log_path))
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
    if args.cmd == 'reanalyse':
        from cchess_alphazero.worker import reanalyse
        return reanalyse.start(config)
    if args.cmd == 'opt':                                   # reference manager.py:85-87
        from cchess_alphazero.worker import optimize
        return optimize.start(config)
    raise SystemExit(f"`run.py {args.cmd}` is not part of the MI355X self-play hot path (SURVEY 8): use the reference "
                     f"implementation for it; the play records written by `run.py self` are in the reference's format")
