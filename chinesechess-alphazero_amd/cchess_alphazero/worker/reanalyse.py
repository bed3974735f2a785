"""``run.py reanalyse`` worker: MuZero's Reanalyse over stored play records.

Every game of every record file under ``--records`` (default ``data_dir/trained``, where ``run.py opt`` moves what it has
trained on) is walked again by the batched engine: the moves and the result stay, every position is searched with the best
model as a self-play ply is searched, and the record's targets -- pi, the training weight, q, s, according to the options
that are on -- are replaced by this run's (lib/reanalyse.py, SelfPlayEngine(script=...)).  One output file per source file,
games in source order, written where ``run.py opt`` looks for play records; a finished source file moves to
``<records>/reanalysed/``.  One device; several GPUs: give each its own directory of files."""
import os
import shutil
import time
from glob import glob
from logging import getLogger

from cchess_alphazero import search_options
from cchess_alphazero.lib import reanalyse as ra
from cchess_alphazero.lib.data_helper import write_game_data_to_file

logger = getLogger(__name__)

PLY_BUDGET = 200000          # plies of scripts handed to the device at once (2 bytes each) unless config.engine says otherwise


def output_name(config, source):
    """The output file's name for a source file: the play-record pattern `run.py opt` globs for."""
    base = os.path.basename(source)
    tmpl = config.resource.play_data_filename_tmpl
    head, tail = tmpl.split("%s")
    return base if base.startswith(head) and base.endswith(tail) else tmpl % os.path.splitext(base)[0]


class ReanalyseWorker:
    """run() walks every file once and returns the totals: dict(files, games, plies, mismatches, skipped, seconds)."""

    def __init__(self, config, model=None, evaluator=None):
        self.config = config
        self.model = model
        self.evaluator = evaluator
        self.engine = None
        ec, rc = config.engine, config.resource
        self.records_dir = getattr(ec, "reanalyse_records", None) or os.path.join(rc.data_dir, "trained")
        self.out_dir = getattr(ec, "reanalyse_out", None) or rc.play_data_dir
        self.ply_budget = int(getattr(ec, "reanalyse_plies", None) or PLY_BUDGET)
        self.done_dir = os.path.join(self.records_dir, "reanalysed")
        if os.path.abspath(self.out_dir) == os.path.abspath(self.records_dir):
            raise ValueError(f"reanalyse: --out {self.out_dir} is the records directory itself")

    def _engine_for(self, scripts):
        if self.engine is not None:
            self.engine.set_script(scripts)
            return self.engine
        import torch
        from cchess_alphazero.engine import SelfPlayEngine
        ec = self.config.engine
        net = self.model.model if self.model is not None else None
        self.engine = SelfPlayEngine(self.config, ec.games_per_gpu, net=net, dtype=getattr(torch, ec.net_dtype),
                                     seed=ec.base_seed, max_nodes_per_game=ec.max_nodes_per_game, pool_chunks=ec.pool_chunks,
                                     max_depth=ec.max_depth, sims_per_round=ec.sims_per_round, evaluator=self.evaluator,
                                     record_visits=True, script=scripts)
        for line in search_options.describe(vars(self.engine), self.config.play.simulation_num_per_move):
            logger.info(f"reanalyse: {line}")
        return self.engine

    def _walk(self, scripts):
        """Rounds until every script has produced its record: {script index: drained game}."""
        eng = self._engine_for(scripts)
        n = len(scripts.z)
        every = max(1, getattr(self.config.engine, "report_every_rounds", 64))
        eng.start(0)
        got = {}
        while len(got) < n:
            for _ in range(every):
                eng.step()
            idle = eng.search.pending() == 0                # (asked before the drain: an idle engine has written everything)
            for g in eng.drain():
                got[g["script_index"]] = g
            if idle and len(got) < n:
                raise RuntimeError(f"reanalyse: the engine went idle with {n - len(got)} of {n} scripts missing "
                                   f"(finished-game ring overrun?)")
        return got

    def run_batch(self, files):
        """One batch: the scripts of `files` on the device together.  Returns dict(games, plies, mismatches, skipped)."""
        t0 = time.time()
        per_file = [ra.load_games(f) for f in files]
        flat = [g for games in per_file for g in games]
        sources = [ra.Source(fi, gi) for fi, games in enumerate(per_file) for gi in range(len(games))]
        scripts, kept, aside = ra.pack_scripts(flat, self.max_len, sources)
        skipped = {src: why for src, why in aside}
        got = self._walk(scripts) if kept else {}
        mismatches = plies = games_out = 0
        by_source = {}
        for k, src in enumerate(kept):
            g = got[k]
            if g["script_mismatch"]:
                mismatches += 1
                skipped[src] = f"the moves do not fit the rules at ply {g['turns']}"
            elif g.get("visits") is None:
                skipped[src] = "visit entries were lost"
            else:
                by_source[src] = g
        os.makedirs(self.out_dir, exist_ok=True)
        os.makedirs(self.done_dir, exist_ok=True)
        for fi, (path, games) in enumerate(zip(files, per_file)):
            out = []
            for gi, game in enumerate(games):
                src = ra.Source(fi, gi)
                if src in skipped:
                    logger.info(f"reanalyse: {path} game {gi} not written: {skipped[src]}")
                    continue
                out += ra.rewrite_game(game, by_source[src]["data"])
                games_out += 1
                plies += len(game) - 1
            if out:
                write_game_data_to_file(os.path.join(self.out_dir, output_name(self.config, path)), out)
            shutil.move(path, os.path.join(self.done_dir, os.path.basename(path)))
        dt = max(time.time() - t0, 1e-9)
        logger.info(f"reanalyse: batch of {len(files)} files: games={games_out} plies={plies} plies/s={plies / dt:.1f} "
                    f"mismatches={mismatches} skipped={len(skipped)}")
        return dict(games=games_out, plies=plies, mismatches=mismatches, skipped=len(skipped))

    @property
    def max_len(self):
        """The longest script the engine's finished-game record holds: max_plies + 1, max_plies = 2 max_game_length + 2."""
        return 2 * int(self.config.play.max_game_length) + 3

    def run(self):
        files = sorted(glob(os.path.join(self.records_dir, "*.json")))
        t0 = time.time()
        total = dict(files=len(files), games=0, plies=0, mismatches=0, skipped=0)
        if not files:
            logger.info(f"reanalyse: no record files in {self.records_dir}")
        sizes = [sum(len(g) - 1 for g in ra.load_games(f)) for f in files]
        for a, b in ra.batches(sizes, self.ply_budget):
            for k, v in self.run_batch(files[a:b]).items():
                total[k] += v
        total["seconds"] = time.time() - t0
        logger.info(f"reanalyse: done: {total}")
        return total

    def close(self):
        if self.engine is not None:
            self.engine.close()
            self.engine = None


def start(config):
    """Entry point of ``run.py reanalyse``: one device, the first of --gpu."""
    import torch
    from cchess_alphazero.worker.self_play import load_model
    torch.cuda.set_device(int(str(config.opts.device_list).split(",")[0]))
    model, _ = load_model(config)
    worker = ReanalyseWorker(config, model=model)
    try:
        return worker.run()
    finally:
        worker.close()
