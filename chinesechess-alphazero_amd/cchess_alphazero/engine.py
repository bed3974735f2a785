"""Batched self-play engine: thousands of concurrent games on one MI355X.

One engine = one GPU = one process.  Each ROUND is
    cz_search_round (hand-written HIP, one wavefront per game: k_sim(BACKUP) -> k_advance -> k_sim(SELECT);
             backup / select / expand / game rules, leaf planes written straight into the evaluation queue)
 -> one ResNet forward over the whole queue (agent/model.py InferenceNet: hand-written MFMA kernels for the input
    layer fused into the first residual block, the residual tower, the head convolutions, the dense heads)
with no host decision and no device->host copy in between.  Finished games are appended to a device
ring and drained by the host only when it wants to write play-record files.

This replaces the reference's process/thread topology (worker/self_play.py:48-60 ProcessPoolExecutor,
agent/player.py ThreadPoolExecutor + sender/receiver threads, agent/api.py prediction thread + pipes).
"""
import os
import time
from logging import getLogger

import torch

from cchess_alphazero import _native, search_options
from cchess_alphazero._native_search import Search
from cchess_alphazero.agent.model import CChessNet, guarded_inference_net
from cchess_alphazero.environment.lookup_tables import ActionLabelsRed
from cchess_alphazero.environment.static_env import INIT_STATE, array_to_state
from cchess_alphazero.lib.data_helper import record_item
from cchess_alphazero.search_options import DRAW_REFUSAL, MOVES_LEFT_REFUSAL

logger = getLogger(__name__)

_PLANES_CODE = {torch.float32: _native.F32, torch.float16: _native.F16, torch.bfloat16: _native.BF16}
# record_visits: the device ring holds 8 plies per game per round for this many rounds (one round records at most 8 plies
# of a game), and the engine moves it to the host this often -- no entry can be dropped
VISIT_DRAIN_ROUNDS = 16


def bytes_per_expansion(mean_depth, mean_edges, mean_leaf_moves):
    """Algorithmic HBM bytes of one node expansion (canonical fp32 accounting):
    13 478 + 14 L + sum_i (16 + 14 C_i) + 28 d."""
    return 13478.0 + 14.0 * mean_leaf_moves + mean_depth * (16.0 + 14.0 * mean_edges) + 28.0 * mean_depth


class SelfPlayEngine:
    def __init__(self, config, n_games, net=None, dtype=torch.float32, device=None, seed=0,
                 max_nodes_per_game=0, pool_chunks=0, max_depth=0, sims_per_round=None, evaluator=None,
                 use_history=False, trunk=None, record_visits=None, book=None, book_rate=None, fast_sims=None,
                 full_rate=None, forced_playouts=None, record_q=None, record_surprise=None, leaf_mirror=None,
                 gumbel=None, gumbel_visit=None, gumbel_scale=None, gumbel_full=None, eval_cache=None, solver=None,
                 kld_gain=None, kld_interval=None, resign_audit=None, script=None, moves_left_slope=None,
                 moves_left_cap=None, draw_score=None, show_wdl=None, lcb=None, lcb_min_visits=None, cpuct_factor=None,
                 cpuct_base=None, policy_temp=None):
        """config: the reference's Config object (config.play.* / config.model.* are read).
        net: a CChessNet (random-init if None).  evaluator: optional callable planes -> (policy, value)
        replacing the network (tests).  trunk: "mfma" (hand-written convolution kernel, the default where the
        filter count allows) or "library" (MIOpen), see agent/model.py InferenceNet.  record_visits: every searched
        ply's root visit counts go into the records (drain: items [move, value, pi]); None = config.engine.record_visits.
        book: start positions (state strings in the mover's frame, lib/book.py load_book; None = the file
        config.engine.book_path, if set): game `game_id` starts from book[game_id % n] with probability book_rate (None =
        config.engine.book_rate), otherwise from INIT_STATE.  The side that moves first plays "red" in every count.
        fast_sims .. kld_interval, record_visits: the search options of search_options.py under their config.engine names
        (None = config.engine's value); that table has each one's meaning, range, prerequisite and the options it cannot run
        beside, and a violation raises its SearchOptionError (a ValueError) before a device is asked for.  What they add to
        drain()'s items: record_visits [move, value, pi], the playout cap a weight (0 for a fast ply), record_q the root's
        search value q, record_surprise the ply's surprise s -- [move, value, pi or None, weight, q or None, s]; with
        forced_playouts pi is the pruned counts, with gumbel softmax(log prior + sigma(completed Q)) scaled to 65536
        (include/czero.h).  eval_cache: every network change empties it (_install).
        resign_audit (None = config.engine.resign_audit; needs record_visits): the max-q record of the search is on --
        every VisitEntry of drain()'s `visits` carries the number its ply's resignation test compared (maxq) and whether
        its game plays on without resignation (no_resign): what lib/resign_audit.py audits.  It is a game-loop option,
        not one of search_options.py's; the records do not change.
        script: games to walk again instead of playing new ones (lib/reanalyse.py pack_scripts: init_boards, labels, offsets,
        z): game id i replays script i, every ply searched as a self-play ply is and only the move taken from the script
        (Search.set_script).  Needs record_visits; refused beside a book, the resignation audit and what
        search_options.SCRIPT_EXCLUDES lists.  start(0): slot g walks scripts g, g + G, ... and goes idle after its last;
        drain() reports `script_index` and `script_mismatch`.
        moves_left_slope, moves_left_cap (None = config.engine's values; slope 0 = off): the moves-left utility of the search
        (Search.set_moves_left).  It is a row of search_options.py's SIDE table, as the next three paragraphs' options are;
        check(moves_left=True) refuses what search_options.MOVES_LEFT_EXCLUDES lists, and a script.  The network must have the moves-left output (`run.py
        opt --moves-left`; a ValueError otherwise, here and in set_network); every forward then also fills
        search.moves_left_x (the tail launch is cz_heads_tail_ml), and the load-time guard and audit_network measure that
        output too.  An evaluator callable returns (policy, value, x).
        draw_score, show_wdl (None = config.engine's values): the draw average of the search (Search.set_draw), on with a draw
        score other than 0 or with show_wdl.  check(draw=True) refuses what
        search_options.DRAW_EXCLUDES lists, a script and the moves-left utility.  The network must have the win / draw / loss
        value head (`run.py opt --value-head wdl`; a ValueError otherwise, here and in set_network); every forward then also
        fills search.wdl_rows, and the load-time guard and audit_network measure the draw probability too.  An evaluator
        callable returns (policy, value, wdl [n, 3]).
        lcb, lcb_min_visits (None = config.engine's values): the lower-confidence-bound move choice (Search.set_lcb), on with
        lcb > 0: from the ply where the temperature reaches 0 a game plays the move with the best lower bound of its value.
        check(lcb=True) refuses what search_options.LCB_EXCLUDES lists, a script, the
        moves-left utility and the draw average.  Every network will do.
        cpuct_factor, cpuct_base, policy_temp (None = config.engine's values): the schedule of c_puct (Search.set_cpuct_schedule,
        on with cpuct_factor > 0) and the policy temperature (Search.set_policy_temperature, on with policy_temp != 1).  Plain
        parameters of the search: they exclude nothing.  The temperature is applied to logits: an evaluator callable, or a
        network that hands over probabilities (engine.policy_logits = False, or one without supports_logits()), is refused
        with a ValueError, here and in set_network."""
        side = search_options.resolve_side(
            config, moves_left_slope=moves_left_slope, moves_left_cap=moves_left_cap, draw_score=draw_score, show_wdl=show_wdl,
            lcb=lcb, lcb_min_visits=lcb_min_visits, cpuct_factor=cpuct_factor, cpuct_base=cpuct_base, policy_temp=policy_temp)
        vars(self).update(side)                # self.moves_left_slope .. self.policy_temp; self.moves_left, self.draw, self.lcb_on, ..
        if self.policy_temp_on and evaluator is not None:
            raise ValueError(search_options.POLICY_TEMP_REFUSAL.format(T=self.policy_temp, who="an evaluator callable"))
        opts = search_options.resolve(
            config, record_visits=record_visits, fast_sims=fast_sims, full_rate=full_rate, forced_playouts=forced_playouts,
            record_q=record_q, record_surprise=record_surprise, leaf_mirror=leaf_mirror, gumbel=gumbel,
            gumbel_visit=gumbel_visit, gumbel_scale=gumbel_scale, gumbel_full=gumbel_full, eval_cache=eval_cache,
            solver=solver, kld_gain=kld_gain, kld_interval=kld_interval)
        search_options.check(opts, history=use_history, script=script is not None, moves_left=self.moves_left,
                             draw=self.draw, lcb=self.lcb_on)
        if self.moves_left and evaluator is None and net is not None and not net.moves_left_head:
            raise ValueError(MOVES_LEFT_REFUSAL.format(slope=self.moves_left_slope))
        if self.draw and evaluator is None and net is not None and not net.wdl_head:
            raise ValueError(DRAW_REFUSAL.format(score=self.draw_score, show_wdl=self.show_wdl))
        self.resign_audit = bool(getattr(getattr(config, "engine", None), "resign_audit", False)
                                 if resign_audit is None else resign_audit)
        if self.resign_audit and not opts["record_visits"]:
            raise ValueError("resign_audit needs record_visits: the max q rides beside the visit entries")
        if script is not None and self.resign_audit:
            raise ValueError("a script excludes resign_audit: a scripted game has no resignation test")
        if script is not None and (book or os.environ.get("CZ_BOOK") or getattr(getattr(config, "engine", None), "book_path", None)):
            raise ValueError("a script excludes a book: every script has its own start position")
        vars(self).update(opts)                # self.record_visits, self.fast_sims, ... self.kld_interval
        _native.require_gpu()
        self.config = config
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        torch.cuda.set_device(self.device)
        self.dtype = dtype
        self.evaluator = evaluator
        self.net = None
        self.trunk = None
        planes_code = _PLANES_CODE[dtype]
        if evaluator is None:
            if net is None:
                torch.manual_seed(0)
                net = CChessNet.from_model_config(config.model)
                if self.moves_left and not net.moves_left_head:
                    raise ValueError(MOVES_LEFT_REFUSAL.format(slope=self.moves_left_slope))
                if self.draw and not net.wdl_head:
                    raise ValueError(DRAW_REFUSAL.format(score=self.draw_score, show_wdl=self.show_wdl))
            self.model_cfg = net.cfg
            if trunk is None:
                trunk = getattr(getattr(config, "engine", None), "net_trunk", "mfma")
            if net.cfg["cnn_filter_num"] not in (32, 128, 192, 256):
                trunk = "library"
            self.trunk = trunk
            self.arith = os.environ.get("CZ_TOWER_ARITH") or getattr(getattr(config, "engine", None), "net_arith", "bf16x3")
            if trunk == "mfma":
                planes_code = _native.U8      # the hand-written input convolution reads the 0/1 planes as bytes
        self.search = Search(config.play, n_games, planes_dtype=planes_code,
                             evaluate=getattr(config.opts, "evaluate", False), seed=seed,
                             max_nodes_per_game=max_nodes_per_game, pool_chunks=pool_chunks, max_depth=max_depth,
                             sims_per_round=sims_per_round, device=self.device, use_history=use_history,
                             pool_fraction=getattr(getattr(config, "engine", None), "pool_fraction", None))
        if self.eval_cache:                    # the table: before the network's buffers, before start() and a graph capture
            self.search.set_eval_cache(self.eval_cache)
        self.policy_logits = False             # (an evaluator callable hands over probabilities, like the reference's pipe)
        self._ref_net = net if evaluator is None else None     # (CPU copy of the weights: audit_network's float64 reference)
        if evaluator is None:
            self._install(net)
        # compact evaluation queue: the network runs only on the slots that hold a new leaf (2-7 % of the slots of a
        # sustained self-play round carry none, more with large K); needs the kernels that read the count on the device
        want = getattr(getattr(config, "engine", None), "compact_queue", True)
        self._want_compact = want
        self.compact = bool(want and self.net is not None and self.net.supports_compact_queue())
        self.rounds = 0
        self.seed = seed
        self._graph = None
        self._since_pull = 0
        if self.record_visits:
            self.search.record_visits(True, capacity=8 * VISIT_DRAIN_ROUNDS * self.search.G)
        if self.resign_audit:                  # beside the visit ring: after it, before start() and a graph capture
            self.search.record_maxq(True)
        ec = getattr(config, "engine", None)
        book_path = os.environ.get("CZ_BOOK") or getattr(ec, "book_path", None)     # (CZ_BOOK: a book for bench.py / the tools)
        if book is None and book_path:
            from cchess_alphazero.lib.book import load_book
            book = load_book(book_path)
        self.book = list(book) if book else []
        self.book_rate = float(getattr(ec, "book_rate", 1.0) if book_rate is None else book_rate)
        if self.book:                                          # handed over before start() and before a graph capture
            from cchess_alphazero.lib.book import book_boards
            self.search.set_book(book_boards(self.book), self.book_rate)
        # every other option that is on: likewise before start() and before a graph capture
        search_options.apply(self.search, opts, skip=("eval_cache",))
        # (the rows of the moves-left utility and the draw average, search.moves_left_x and search.wdl_rows, are allocated here:
        #  fixed for a graph capture)
        search_options.apply_side(self.search, side)
        if self.cpuct_on:
            logger.info(search_options.CPUCT_LOG.format(cpuct_factor=self.cpuct_factor, cpuct_base=self.cpuct_base))
        if self.policy_temp_on:                # (after _install: the rows are logits by now, or _install has refused)
            self.search.set_policy_temperature(self.policy_temp)
            logger.info(search_options.POLICY_TEMP_LOG.format(policy_temp=self.policy_temp))
        self.script = script
        if script is not None:                 # last: the library checks it against everything that is on
            self.search.set_script(*script)

    def _build_net(self, net):
        """The inference network for these weights with the tower arithmetic checked against float64 (agent/model.py
        guarded_inference_net): engine.net_arith is the REQUEST, .arith_effective what the weights allow.  Nothing of the
        engine changes here: a guard that raises (out of memory, a damaged weight file) leaves the games on the old network."""
        guard = getattr(getattr(self.config, "engine", None), "arith_guard", True)
        return guarded_inference_net(net, self.dtype, trunk=self.trunk, arith=self.arith, device=self.device,
                                     guard=None if guard else False, moves_left=self.moves_left, draw=self.draw)

    def _install(self, net, built=None):
        self.net = built if built is not None else self._build_net(net)
        self.net_arith_effective = self.net.arith_effective
        self.net_calibration = self.net.calibration
        # the one place every network change passes through (construction, set_network, the rebuild after demote_arith):
        # what the evaluation cache holds was the old network's
        self.search.clear_eval_cache()
        # the engine's own queue: raw logits instead of a softmax over all 2086 columns (the search spreads the priors over
        # the legal moves anyway, reference player.py:272-283: the denominator cancels) -- engine.policy_logits = False opts out
        want = getattr(getattr(self.config, "engine", None), "policy_logits", True)
        self.policy_logits = bool(want and self.net.supports_logits())
        if self.policy_temp_on and not self.policy_logits:
            raise ValueError(search_options.POLICY_TEMP_REFUSAL.format(
                T=self.policy_temp, who="this network" if want else "a network with engine.policy_logits = False"))
        self.search.policy_logits(self.policy_logits)
        # the leaves' occupancy boards beside their planes: the fused input layer takes them directly (engine.leaf_masks = False
        # opts out; only the hand-written trunk on byte planes reads them)
        want_m = getattr(getattr(self.config, "engine", None), "leaf_masks", True) and os.environ.get("CZ_LEAF_MASKS", "1") != "0"
        use_m = bool(want_m and self.trunk == "mfma" and self.search.planes.dtype == torch.uint8)
        self.search.leaf_masks(use_m)
        # ... and where the network reads NOTHING but the boards (input layer fused into the first block) the kernel stops
        # writing the planes: a leaf costs a code row + two word stores instead of the 1260-element encoder pass
        # (engine.leaf_planes = True or CZ_LEAF_PLANES=1 keeps them; queue_planes() rebuilds rows for the audits either way)
        keep_p = getattr(getattr(self.config, "engine", None), "leaf_planes", False) or os.environ.get("CZ_LEAF_PLANES", "0") == "1"
        if use_m:
            self.search.leaf_planes(bool(keep_p or not self.net.takes_masks(self.search.planes.dtype)))

    # ---- control ----
    def set_network(self, net):
        """Swap the weights the games are played with (hot reload of the best model, reference agent/api.py:76-87):
        rebuilds the inference network; a captured HIP graph holds the old weights' buffers and is captured again.
        The new network is built and measured FIRST (the float64 calibration allocates a few hundred MB beside a
        search pool that owns most of HBM): if that raises, the engine keeps playing on the old weights -- and its graph --
        and the exception goes to the caller."""
        if self.evaluator is not None:
            raise RuntimeError("the engine was built on an evaluator callable, not on a network")
        # (the value head's end is not part of what must match: each InferenceNet carries its own tail and hands the search
        #  one scalar per leaf, so a scalar net may follow a win / draw / loss one and the other way round)
        #  (nor is the moves-left output -- unless the moves-left utility reads it: then the new network needs it too, and is
        #  refused before anything is touched, the way a guard failure is: the games stay on the old network)
        same = lambda cfg: {k: v for k, v in cfg.items() if k not in ("value_outputs", "moves_left")}
        if same(net.cfg) != same(self.model_cfg):
            raise ValueError(f"hot reload: topology changed ({self.model_cfg} -> {net.cfg})")
        if self.moves_left and not net.moves_left_head:
            raise ValueError("hot reload: " + MOVES_LEFT_REFUSAL.format(slope=self.moves_left_slope))
        if self.draw and not net.wdl_head:     # (likewise the draw average and the win / draw / loss head)
            raise ValueError("hot reload: " + DRAW_REFUSAL.format(score=self.draw_score, show_wdl=self.show_wdl))
        torch.cuda.synchronize(self.device)
        built = self._build_net(net)                           # may raise: nothing has been touched yet
        if self.policy_temp_on and not built.supports_logits():    # (likewise the policy temperature and logit rows)
            raise ValueError("hot reload: " + search_options.POLICY_TEMP_REFUSAL.format(T=self.policy_temp, who="this network"))
        had_graph = self._graph is not None
        self._graph = None
        torch.cuda.synchronize(self.device)
        self._install(net, built)
        self._ref_net = net
        self.compact = bool(self._want_compact and self.net.supports_compact_queue())
        if had_graph:
            self.capture_graph()

    def set_resign_threshold(self, t):
        """Replace config.play.resign_threshold for every ply whose move is chosen after the call
        (Search.set_resign_threshold).  The threshold is an argument of the kernels: a captured HIP graph holds the old
        value and is captured again, the way set_network does it.  The games and their trees are not touched."""
        t = float(t)
        if t != t or t in (float("inf"), float("-inf")):
            raise ValueError(f"set_resign_threshold: {t} is not finite")
        torch.cuda.synchronize(self.device)
        had_graph = self._graph is not None
        self._graph = None
        self.search.set_resign_threshold(t)
        if had_graph:
            self.capture_graph()

    @property
    def resign_threshold(self):
        return self.search.resign_threshold

    def queue_planes(self, n=64):
        """The first n positions of the evaluation queue as planes (a copy) -- rebuilt from the occupancy boards when the
        search kernel writes only those (Search.queue_planes)."""
        return self.search.queue_planes(n)

    def audit_network(self, n=64):
        """Re-measure the running arithmetic on LIVE queue positions (the load-time calibration set is random
        playouts; the positions a search actually asks about are more tactical).  Takes up to n of the positions the last round
        asked about -- the compact queue's rows q_rows[:q_count]; slots that were never written (empty boards) are dropped --,
        evaluates the float64 reference and the running network on them and returns measure_against_reference's figures + `ok`
        (within_guard: policy / value within GUARD_TOL, logits within LOGIT_TOL) + `positions`.  With a leaf mirror
        (leaf_mirror) some of those rows hold mirrored positions: both networks are given the same rows, so the comparison
        needs no flags.  A failing audit is logged; the
        caller decides (worker/self_play.py asks for the next more exact arithmetic and rebuilds the network through the
        load-time guard on its standard calibration set)."""
        from cchess_alphazero.agent.model import measure_against_reference, reference_forward_f64, within_guard
        if self.net is None or getattr(self, "_ref_net", None) is None:
            return None
        rows = None
        if getattr(self.search, "q_rows", None) is not None:
            cnt = min(int(self.search.q_count.item()), int(n))
            if cnt > 0:
                rows = self.search.q_rows[:cnt].long()
        planes = self.search.queue_planes(rows=rows) if rows is not None else self.queue_planes(n)
        if planes.dtype != torch.uint8:
            planes = (planes != 0).to(torch.uint8)
        planes = planes[planes.flatten(1).ne(0).any(1)].contiguous()          # (a slot no leaf was ever written to is an empty board)
        if planes.shape[0] == 0:
            return None
        ref = reference_forward_f64(self._ref_net, planes, with_wdl=self.draw, with_moves_left=self.moves_left)
        m = measure_against_reference(self.net, ref, planes, moves_left_ref=ref[-1] if self.moves_left else None,
                                      draw_ref=ref[-1][:, 1] if self.draw else None)     # (never both: they exclude each other)
        m["ok"] = within_guard(m)
        m["arith"] = self.net_arith_effective
        m["positions"] = int(planes.shape[0])
        if not m["ok"]:
            logger.warning("live-queue audit: arithmetic %s is outside the guard on %d live positions: %s",
                           self.net_arith_effective, planes.shape[0], m)
        return m

    def demote_arith(self):
        """Lower the REQUESTED tower arithmetic one step towards exactness below what is running now (one reduced block
        fewer -- c6 -> c6>N-1 -> ... -> c6>1 -> c8 -> c8>N-1 -> ... -> f16x3 -> bf16x3; agent/model.py next_more_exact); the
        next _build_net / set_network starts its guard there.  False when there is nothing below."""
        from cchess_alphazero.agent.model import next_more_exact
        cur = self.net_arith_effective or "bf16x3"
        nxt = next_more_exact(cur, len(self.net.res)) if cur.split(">")[0] in ("c6", "c8", "f16x3") else None
        if nxt is None:
            return False
        self.arith = nxt
        return True

    def set_script(self, script):
        """The next scripts of an engine created with one (worker/reanalyse.py: one call per batch); start(0) begins them.  A
        captured graph holds the old scripts' addresses and is dropped."""
        if self.script is None:
            raise ValueError("set_script: the engine was created without a script (SelfPlayEngine(script=...))")
        self.search.set_script(*script)
        self.script = script
        self._graph = None

    def start(self, first_game_id=0, game_id_stride=0):
        self.search.start_selfplay(self.seed, first_game_id, game_id_stride)

    def prewarm(self, max_iters=8, max_seconds=90.0):
        """Run the network on the (idle) queue until its time settles: MIOpen picks / compiles its solvers on
        the first calls of a new shape (seconds, with naive fallback kernels meanwhile).  Initialisation only.
        Returns the list of forward times (s)."""
        times = []
        if self.net is None:
            return times
        import time as _t
        t_begin = _t.perf_counter()
        for _ in range(max_iters):
            torch.cuda.synchronize(self.device)
            t0 = _t.perf_counter()
            self.net(self.search.planes)
            torch.cuda.synchronize(self.device)
            times.append(_t.perf_counter() - t0)
            if len(times) >= 2 and 0.8 * times[-2] < times[-1] < 1.25 * times[-2]:
                break
            if _t.perf_counter() - t_begin > max_seconds:
                break
        return times

    def _round(self):
        self.search.round(compact=self.compact)

    def _forward(self):
        s = self.search
        if self.evaluator is not None:
            p, v, *x = self.evaluator(s.planes)
            if self.moves_left:
                s.moves_left_x.copy_(x[0])
            if self.draw:
                s.wdl_rows.copy_(x[0])
        else:
            out = (s.policy, s.value)
            ml = s.moves_left_x if self.moves_left else None   # (the rows of `value`: by slot, or by compact row)
            kw = dict(wdl=s.wdl_rows) if self.draw else {}     # (likewise: the draw average's rows)
            if self.compact:
                p, v = self.net(s.planes, rows=s.q_rows, count=s.q_count, out=out, logits=self.policy_logits, masks=s.masks,
                                moves_left=ml, **kw)
            else:
                p, v = self.net(s.planes, out=out, logits=self.policy_logits, masks=s.masks, moves_left=ml, **kw)
            if p is s.policy:                                  # written in place (the hand-written network path)
                return
        s.policy.copy_(p)
        s.value.copy_(v)

    def step(self):
        """One lock-step round for every game: tree kernel, then the network on the evaluation queue."""
        if self._graph is not None:
            self._graph.replay()
        else:
            self._round()
            self._forward()
        self.rounds += 1
        if self.record_visits:
            # the entries fetched by the previous pull are sorted while this round runs; a pull itself waits for the
            # device, so the host work is kept out of that gap
            self.search.ingest_visits()
            self._since_pull += 1
            if self._since_pull >= VISIT_DRAIN_ROUNDS:
                self.search.pull_visits(defer=True)
                self._since_pull = 0

    def capture_graph(self, warmup=2):
        """Capture kernel + network forward of one round into a HIP graph (no host work per round)."""
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._round()
                self._forward()
                self.rounds += 1
        torch.cuda.current_stream(self.device).wait_stream(side)
        if self.record_visits:
            self.search.pull_visits()
            self._since_pull = 0
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._round()
            self._forward()
        self.rounds += 1          # capture does not execute; the first replay does
        self._graph = g

    def counters(self):
        return self.search.counters()

    def drain(self, max_records=4096):
        """Finished games since the last call, as the reference's play-record lists
        ([init_state, [move, value], ...], self_play.py:202-208) plus metadata.  Element 0 is the game's real first state:
        INIT_STATE, or the book position (mover's frame) the kernel started it from -- `book_index`, None for INIT_STATE;
        the values alternate from the first mover's view ("red").  With record_visits a searched move's
        item is [move, value, pi] (lib/data_helper.py pi_from_visits); the appended king capture, and every move of a game
        whose visit record is incomplete (`visits` None), keep the two-element form.  With a playout cap (fast_sims) the
        item of a FAST ply is [move, value, pi or None, 0]: element 2 is pi where a full ply would carry it, else None;
        element 3 is the row's training weight (lib/replay_window.py keeps the position, the trainer skips the row).  A
        full ply's item is unchanged.  `fast_plies` counts the game's fast plies.  With forced playouts
        pi comes from the pruned counts; `pruned_visits` is the number of root visits pruning removed from the game's
        entries, sum of raw_total - sum of the non-banned pruned counts (0 without forced playouts).  With record_q the
        item of every ply that has a visit entry is [move, value, pi or None, weight, q] (lib/data_helper.py record_item):
        weight 1 on a full ply and 0 on a fast one, q the root's search value rounded to 6 places or None; the appended
        king capture, a resignation and games whose visit record is incomplete keep the shorter forms.  With
        record_surprise such an item is [move, value, pi or None, weight, q or None, s]: s the ply's policy surprise
        rounded to 6 places or None, q None with record_q off.
        A scripted game (script_index: its script, None otherwise) has the script's start position, its moves and, as
        `value`, its z.  script_mismatch: the script did not fit the rules, the game holds the moves applied before that
        and store is False."""
        out = []
        for r in self.search.drain_records(max_records, with_visits=self.record_visits):
            v = r["value"]
            vis = r.get("visits")
            bi = r["book_index"]
            si = r["script_index"]
            data = [array_to_state(self.script[0][si]) if si is not None else INIT_STATE if bi is None else self.book[bi]]
            for i, m in enumerate(r["moves"]):
                e = vis[i] if vis is not None and i < len(vis) and not vis[i].resign else None
                data.append(record_item(ActionLabelsRed[int(m)], v if i % 2 == 0 else -v, e, r["fast"][i], self.record_q,
                                        ActionLabelsRed, record_surprise=self.record_surprise))
            pruned = [e for e in vis or [] if e.pruned]
            out.append(dict(game_id=r["game_id"], turns=r["turns"], value=v, store=r["store"],
                            resigned=r["resigned"], book_index=bi, script_index=r["script_index"],
                            script_mismatch=r["script_mismatch"], fast_plies=sum(r["fast"]),
                            pruned_visits=sum(e.raw_total - int(e.n[~e.banned].sum()) for e in pruned), data=data))
            if self.record_visits:
                out[-1]["visits"] = vis
        return out

    def close(self):
        self.search.close()
