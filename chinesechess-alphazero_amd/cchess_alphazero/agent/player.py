"""``CChessPlayer`` with the reference's constructor / ``action`` / ``close`` contract
(cchess_alphazero/agent/player.py:36-196), backed by the gfx950 search kernels.

One player owns one device search object with a single game tree (external mode of
``cz_search_*``).  Search, virtual loss, transposition table, prior spreading, PUCT, backup, policy
and temperature sampling all run on the GPU; this class only moves the position in and the result out.
The throughput path is ``cchess_alphazero.engine.SelfPlayEngine`` (thousands of games per launch);
this class is the drop-in for callers that drive one game at a time.
"""
from logging import getLogger

import numpy as np

from cchess_alphazero import _native, search_options
from cchess_alphazero._native_search import MAX_NO_ACT, Search
from cchess_alphazero.environment import static_env as senv
from cchess_alphazero.environment.lookup_tables import ActionLabelsRed, label_index

logger = getLogger(__name__)

INFINITE_SIMS = 100000        # `go infinite` (player.py:162-163)


class ActionState:
    def __init__(self, n=0, w=0.0, p=0.0):
        self.n, self.w, self.p = n, w, p
        self.q = w / n if n else 0


class VisitState:
    def __init__(self):
        self.a = {}
        self.sum_n = 0
        self.legal_moves = None
        self.p = None
        self.waiting = False
        self.visit = []
        self.w = 0


class MovesLeftUnavailable(ValueError):
    """The moves-left utility was asked for and the network behind the pipe has no moves-left output."""


MOVES_LEFT_REFUSAL = search_options.MOVES_LEFT_REFUSAL


class DrawUnavailable(ValueError):
    """The draw average was asked for and the network behind the pipe has the scalar value head."""


class PolicyTempUnavailable(ValueError):
    """A policy temperature was asked for and the pipe hands the search probabilities: the temperature is applied to logits."""


class CChessPlayer:
    def __init__(self, config, search_tree=None, pipes=None, play_config=None, enable_resign=False,
                 debugging=False, uci=False, use_history=False, side=0, solver=None, smart_pruning=None,
                 moves_left_slope=None, moves_left_cap=None, draw_score=None, show_wdl=None, lcb=None, lcb_min_visits=None,
                 cpuct_factor=None, cpuct_base=None, policy_temp=None):
        import torch
        self.config = config
        self.play_config = play_config or self.config.play
        self.labels_n = len(ActionLabelsRed)
        self.labels = ActionLabelsRed
        self.move_lookup = {m: i for i, m in enumerate(self.labels)}
        self.pipe = pipes
        self.tree = search_tree if search_tree is not None else {}
        self.enable_resign = enable_resign
        self.debugging = debugging
        self.uci = uci
        self.side = side
        self.search_results = {}
        self.debug = {}
        self.done_tasks = 0
        self.root_state = None
        self.no_act = None
        self.increase_temp = False
        self.use_history = use_history
        self.job_done = False
        self.out = None                      # where `info depth ...` lines go (None: sys.stdout)
        self.last_action = None
        import threading
        self._idle = threading.Event()
        self._idle.set()
        if pipes is None:
            raise ValueError("CChessPlayer needs a pipe to the network (model.get_pipes())")
        # MCTS solver and unreachable-lead stop (search_options.py): None = config.engine's value, off by default.  After
        # action() self.proof is the root's (status, d) -- (0, 0) while the solver is off or nothing is proven.
        opts = search_options.resolve(config, solver=solver, smart_pruning=smart_pruning)
        # The side options (search_options.py SIDE): None = config.engine's value, off by default.  The moves-left utility: the
        # pipe's network must have the output (MovesLeftUnavailable otherwise, before a device is asked for).  The draw average:
        # on with a draw score or with show_wdl, which adds `wdl W D L` to the info lines; the pipe's network must have the
        # win / draw / loss head (DrawUnavailable otherwise).  The lower-confidence-bound move choice and the c_puct schedule:
        # every network will do.  The policy temperature: the pipe hands over probabilities (the reference's protocol), in
        # which a temperature cannot be applied: PolicyTempUnavailable, before a device is asked for.
        side = search_options.resolve_side(
            config, moves_left_slope=moves_left_slope, moves_left_cap=moves_left_cap, draw_score=draw_score, show_wdl=show_wdl,
            lcb=lcb, lcb_min_visits=lcb_min_visits, cpuct_factor=cpuct_factor, cpuct_base=cpuct_base, policy_temp=policy_temp)
        vars(self).update(side)                # self.moves_left_slope .. self.policy_temp; self.moves_left, self.draw, self.lcb_on, ..
        self.last_wdl = None                   # show_wdl: (W, D, L) in permille of the move action() chose
        search_options.check(opts, moves_left=self.moves_left, draw=self.draw, lcb=self.lcb_on)
        if self.policy_temp_on:
            raise PolicyTempUnavailable(search_options.POLICY_TEMP_REFUSAL.format(T=self.policy_temp, who="the player's pipe"))
        if self.moves_left and not getattr(pipes, "moves_left_head", False):
            raise MovesLeftUnavailable(MOVES_LEFT_REFUSAL.format(slope=self.moves_left_slope))
        if self.draw and not getattr(pipes, "wdl_head", False):
            raise DrawUnavailable(search_options.DRAW_REFUSAL.format(score=self.draw_score, show_wdl=self.show_wdl))
        vars(self).update(opts)                # self.solver, self.smart_pruning
        pc = self.play_config
        # simulation count from play_config, lock-step batch from config.play (player.py:155-174)
        merged = type("PC", (), dict(vars(pc)))()
        merged.search_threads = self.config.play.search_threads
        dt = _native.F32
        self._search = Search(merged, 1, planes_dtype=dt, evaluate=getattr(config.opts, "evaluate", False),
                              seed=int(np.random.randint(0, 2 ** 31 - 1)),
                              # one game: a quarter of a GiB of tree at most (`go infinite` reserves 100000 nodes)
                              max_nodes_per_game=600000 if uci else
                              (getattr(getattr(config, "engine", None), "max_nodes_per_game", 0) or 0),
                              pool_chunks=256 if uci else 0,
                              use_history=use_history)
        self._torch = torch
        self.proof = (0, 0)
        search_options.apply(self._search, opts)
        search_options.apply_side(self._search, side)

    # -- network access: device fast path, or the reference's pipe protocol --
    def _evaluate(self, planes, moves_left=False, wdl=False):
        """(policy, value) of the planes; moves_left (the utility is on: a device pipe whose network has the output): a third
        tensor, the raw moves-left output; wdl (the draw average is on: likewise): the win / draw / loss rows [n, 3]."""
        if moves_left:
            return self.pipe.evaluate_device(planes, moves_left=True)
        if wdl:
            return self.pipe.evaluate_device(planes, wdl=True)
        if hasattr(self.pipe, "evaluate_device"):
            return self.pipe.evaluate_device(planes)
        self.pipe.send(list(planes.float().cpu().numpy()))
        while not self.pipe.poll(0.001):
            pass
        rets = self.pipe.recv()
        t = self._torch
        p = t.from_numpy(np.stack([np.asarray(r[0], dtype=np.float32) for r in rets])).to(planes.device)
        v = t.tensor([float(r[1]) for r in rets], dtype=t.float32, device=planes.device)
        return p, v

    def close(self, wait=True):
        self.job_done = True
        if getattr(self, "_search", None) is not None:
            self._search.close()
            self._search = None

    # -- helpers ---------------------------------------------------------------------------------------------------
    def _node(self, stats):
        """VisitState of game 0 from a root_stats / node_stats dict (None when the position is not in the tree)."""
        c = int(stats["counts"][0])
        if c == 0:
            return None
        node = VisitState()
        node.sum_n = int(stats["sum_n"][0])
        node.legal_moves = [self.labels[int(m)] for m in stats["moves"][0, :c]]
        for j, mov in enumerate(node.legal_moves):
            node.a[mov] = ActionState(int(stats["n"][0, j]), float(stats["w"][0, j]), float(stats["p"][0, j]))
        return node

    def _root_value(self, state, hist):
        """debugging=True: the network's (policy, value) of the root, what the reference keeps in self.debug[state]
        (player.py:332-336) and its UCI front-end prints as the score (uci.py:291-292)."""
        t = self._torch
        if self.use_history:
            # a history model always gets 28 planes (expand_and_evaluate, player.py:326-333: state_history_to_planes
            # whether or not the history is long enough; planes 14-27 stay zero without a position two plies back)
            planes = senv.state_history_to_planes(state, hist or [])
        else:
            planes = senv.state_to_planes(state)
        p, v = self._evaluate(t.from_numpy(np.asarray(planes, dtype=np.float32)[None]).cuda())
        return p[0].float().cpu().numpy(), float(v[0])

    def root_wdl(self, label, stats=None):
        """show_wdl: (W, D, L) in permille of the root edge with the move label `label`, for the side to move (uci.wdl_permille);
        None while the option is off, for a move that is not a root edge and for an edge without a visit."""
        if not (self.draw and self.show_wdl):
            return None
        from cchess_alphazero.uci import wdl_permille
        st = stats if stats is not None else self._search.root_stats()
        dr = self._search.node_draws()
        hit = np.nonzero(st["moves"][0, :int(st["counts"][0])] == int(label))[0]
        if not len(hit):
            return None
        j = int(hit[0])
        return wdl_permille(float(st["w"][0, j]), int(st["n"][0, j]), int(dr["dsum"][0, j]), int(dr["dn"][0, j]))

    def principal_variation(self, state, no_act=None, max_len=20):
        """Most-visited line from the root (print_depth_info, player.py:408-433: `>=` keeps the LAST maximum; banned
        moves are skipped at the root only; the line ends at a node that was never selected from).  One kernel launch
        (cz_search_pv; the bans are those of the running search).  Returns the moves in the mover's frame of each ply."""
        return [self.labels[m] for m in self._search.pv(max_len)[0]]

    def print_depth_info(self, state, turns, start_time, value, no_act):
        """`info depth .. score .. time .. pv .. nps ..` (player.py:408-450)."""
        import sys
        from time import time
        from cchess_alphazero.environment.lookup_tables import flip_move
        depth = self.done_tasks // 100
        pv = ""
        t = turns
        end_state = state
        line = [state]                                       # the search path of the line: [s0, m1, s1, m2, s2, ...]
        labels, visits = self._search.pv(20, with_visits=True)
        labels, visits = labels[0], visits[0]
        for lab in labels:
            mov = self.labels[lab]
            pv += " " + senv.to_uci_move(flip_move(mov) if t % 2 == 1 else mov)
            end_state = senv.step(end_state, mov)
            line += [mov, end_state]
            t += 1
        # the reference prints the network value of the position at the END of the line (self.debug holds every
        # evaluated state when debugging, :442-445), seen from `side`; a line that ends on a position the network
        # never saw (terminal, an unvisited move, or debugging off) keeps the root's value as it was passed in, un-negated
        if self.debugging and labels and visits[-1] > 0 and not senv.done(end_state)[0]:
            leaf_v = None
            if visits[-1] == 1:
                # visited once = (almost always) expanded and evaluated by that visit: the edge's W is exactly minus that
                # evaluation (the value the network gave with the history planes of the path it was first reached by) -- no
                # forward, no re-encoding, and equal to what the reference kept in self.debug[state]: the recorded reference
                # scores of tests/golden/uci_k1.json are reproduced this way, history models included.
                # Known limit: when the end node had been created through ANOTHER path before this edge's
                # single visit, that visit descended further and W holds the deeper value, where the reference prints the
                # end node's own network value.  The tree does not record which edge created a node, and the obvious
                # proxies reject valid lines (requiring "nothing selected from the end node yet" breaks two of the recorded
                # reference cases: a later transposition into the node is indistinguishable).  Debug / info line only.
                st = self._search.node_stats(labels[:-1]) if len(labels) > 1 else self._search.root_stats()
                c = int(st["counts"][0])
                hit = np.nonzero(st["moves"][0, :c] == labels[-1])[0]
                if len(hit) and int(st["n"][0, hit[0]]) == 1:
                    leaf_v = -float(st["w"][0, hit[0]])
            if leaf_v is None:
                # (simulations in flight through this edge, K > 1: evaluate the position; a history model gets the
                #  planes of the position two plies up the line, :331-333)
                leaf_v = self._root_value(end_state, line)[1]
            value = leaf_v
            if t % 2 != self.side:
                value = -value
        duration = max(time() - start_time, 1e-9)
        nps = int(depth * 100 / duration) * 1000
        wdl = self.root_wdl(labels[0]) if len(labels) else None      # (the reported move: the line's first)
        shown = f"{int(value * 1000)}" + (" wdl {} {} {}".format(*wdl) if wdl else "")
        out = f"info depth {depth} score {shown} time {int(duration * 1000)} pv" + pv + f" nps {nps}"
        stream = self.out or sys.stdout
        print(out, file=stream)
        logger.debug(out)
        stream.flush()

    def action(self, state, turns, no_act=None, depth=None, infinite=False, hist=None, increase_temp=False):
        from time import time
        t = self._torch
        s = self._search
        base_sims = int(self.play_config.simulation_num_per_move)
        # action(depth=...): that many simulations; infinite: 100000 (player.py:160-163), ended by
        # close_and_return_action from another thread
        s.set_sims(INFINITE_SIMS if infinite else (int(depth) if depth else base_sims))
        self.root_state, self.no_act, self.increase_temp = state, no_act, increase_temp
        self._idle.clear()
        try:
            board = t.from_numpy(senv.state_to_array(state)[None]).cuda()
            na = np.full((1, MAX_NO_ACT), 0xFFFF, dtype=np.uint16)
            bans = list(dict.fromkeys(no_act or []))           # (a move banned twice is banned once)
            if len(bans) > MAX_NO_ACT:                         # the reference's list is unbounded; never truncate silently
                raise ValueError(f"CChessPlayer.action: {len(bans)} banned moves, the engine holds {MAX_NO_ACT}")
            for k, m in enumerate(bans):
                na[0, k] = label_index(m)
            prev, kind = None, None
            if self.use_history and hist:                      # action(hist=...): player.py:150-151, :217-218
                if len(hist) >= 5:
                    prev = t.from_numpy(senv.state_to_array(hist[-5])[None]).cuda()
                    kind = t.tensor([1], dtype=t.uint8, device="cuda")
                else:
                    kind = t.tensor([2], dtype=t.uint8, device="cuda")
            s.set_roots(board, prev_boards=prev, hist_kind=kind,
                        turns=t.tensor([turns], dtype=t.int32, device="cuda"),
                        no_act=t.from_numpy(na.view(np.int16)).cuda().view(t.uint16),
                        n_no_act=t.tensor([len(bans)], dtype=t.uint8, device="cuda"),
                        increase_temp=t.tensor([1 if increase_temp else 0], dtype=t.uint8, device="cuda"),
                        enable_resign=t.tensor([1 if self.enable_resign else 0], dtype=t.uint8, device="cuda"))
            if self.debugging:
                self.debug[state] = self._root_value(state, hist)
            c_before = s.counters()
            before = c_before["sims"]
            start_time, shown, stopped = time(), 0, False
            while True:
                s.round()
                pending, rows = s.leaf_rows()
                if pending == 0:
                    break
                if rows.numel():                               # exactly the positions the reference would send (:112-120)
                    p, v, *x = self._evaluate(s.planes.index_select(0, rows), moves_left=self.moves_left, wdl=self.draw)
                    s.policy.index_copy_(0, rows, p.float())
                    s.value.index_copy_(0, rows, v.float())
                    if x and self.draw:
                        s.wdl_rows.index_copy_(0, rows, x[0].float())
                    elif x:
                        s.moves_left_x.index_copy_(0, rows, x[0].float())
                if self.job_done and not stopped:
                    s.stop()                                   # the next round backs up what is in flight
                    stopped = True
                if self.uci and not stopped:
                    self.done_tasks = s.counters()["sims"] - before
                    if self.done_tasks // 100 != shown:
                        shown = self.done_tasks // 100
                        self.print_depth_info(state, turns, start_time, self.debug.get(state, (None, 0.0))[1], no_act)
            c_after = s.counters()
            self.done_tasks = c_after["sims"] - before
            lost = c_after["overflow_sims"] - c_before["overflow_sims"]
            if lost:                                           # the tree memory of this player ran out: say so
                logger.warning(f"search of {state}: {lost} simulations found no tree memory and backed up 0 "
                               f"(tree_resets {c_after['tree_resets'] - c_before['tree_resets']}); "
                               f"raise engine.max_nodes_per_game / pool_chunks")
            if self.uci and not stopped and self.done_tasks // 100 != shown:      # the last batch reports too
                self.print_depth_info(state, turns, start_time, self.debug.get(state, (None, 0.0))[1], no_act)
            st = s.root_stats()
            c = int(st["counts"][0])
            policy = np.zeros(self.labels_n)
            node = self._node(st) or VisitState()
            for mov, a in node.a.items():
                policy[self.move_lookup[mov]] = 0 if (no_act and mov in no_act) else a.n
            self.tree[state] = node
            if self.debugging:
                order = sorted(node.a.items(), key=lambda kv: -kv[1].n)[:5]
                self.search_results = {m: (a.n, a.q, a.p) for m, a in order}
            if self.solver:
                pr = s.node_proof()
                self.proof = (max(0, int(pr["status"][0])), int(pr["dist"][0]))
            action = int(s.choose([float(np.random.random_sample())])[0])
            self.last_action = self.labels[action] if action >= 0 else None
            self.last_wdl = self.root_wdl(action, st) if action >= 0 else None
            if action < 0:
                return None, list(policy)                      # resign: un-normalised counts (player.py:189-190)
            # the node behind the chosen move, for callers that read it from the tree they passed in
            # (ponder move, uci.py:312-318)
            child = self._node(s.node_stats([action]))
            if child is not None:
                self.tree[senv.step(state, self.labels[action])] = child
            total = policy.sum()
            if total > 0:
                policy /= total
            return self.labels[action], list(policy)
        finally:
            self._idle.set()

    def close_and_return_action(self, state, turns, no_act=None):
        """UCI `stop` (player.py:88-106): end the running search and answer from what has been searched so far.
        Returns (action, value, depth) -- with the MCTS solver on (action, value, depth, proof) -- or None when the
        player resigns."""
        self.job_done = True
        self._idle.wait()                                      # the searching thread finishes its in-flight batch
        node = self.tree.get(state)
        if node is None or not node.a:
            return None
        if state in self.debug:
            _, value = self.debug[state]
        else:
            value = 0
        # the search thread's own choice (same calc_policy / temperature / sampling path) is in last_action
        if self.last_action is None:
            return None
        if self.solver:                                        # (the UCI front-end prints `score mate N` from it)
            return self.last_action, value, self.done_tasks // 100, self.proof
        return self.last_action, value, self.done_tasks // 100
