"""Model-vs-model match play and Elo ratings on the HIP path: the evaluation side of the RainbowDQN loop.

``DeviceArena`` plays ``num_games`` lock-stepped games between a maker player and a breaker player as a closed device loop --
per ply: observation (``hexgnn_env_observe``) -> the mover's Q-network forward (advantages only) -> ``hexgnn_arena_ply``
(pick by argmax / softmax draw / uniform draw, play, dead-and-captured removal, winner, record) -> graph sizes prefix-summed on
the device -- with ``chunk`` plies captured as one HIP graph and ONE word (the number of undecided games) read back per chunk.
``Elo_handler`` is the drop-in for ``GN0/RainbowDQN/evaluate_elo.py``'s class of that name on top of it: same method names and
signatures, the same two-leg match over the shuffled unique opening moves, the same rating arithmetic.

Finished games rest in place (their env restarts and its side flag keeps flipping with everyone else's, so the batched
observation stays uniform); they still pass through the forward until the last game of the batch ends.  There is no CPU
fallback: CNN / Gao / MoHex players, SGF export and ``CachedGraphNorm`` models are refused.

A player with a ``search_scores(env_handle, obs, active)`` method (``gnn_hex_amd.search.SearchPlayer``) takes the place of the
forward: it gets the root env handle, the root observation and the int32 mask of undecided games (computed on the device from
the game records) and returns one score per observation row -- the root visit counts of a PUCT tree search -- from which
``hexgnn_arena_ply`` picks as from a model's output: the most visited move by first maximum, or at ``temperature`` T > 0 a
draw from softmax(count / T) (not count ** (1 / T)).  A search reads leaf sizes back inside a ply, so it needs
``DeviceArena(graph=False)``; with ``graph=True``, ``play`` raises ``ValueError``.  Every ply searches a fresh tree unless the
player keeps the played move's subtree (``SearchPlayer(reuse_tree=True)``): a player with ``begin_match()`` and
``observe_moves(moves)`` is told when a match begins and, after every ply, which vertex each game played (-1: the game rests).
"""
from __future__ import annotations

import os
import random
from collections import defaultdict
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib, ops
from .multi_env_manager import Env_manager
from .observation import ObsTarget, acting_forward, live_norm_of

PICK_GREEDY, PICK_UNIFORM, PICK_SOFTMAX = 0, 1, 2      # HEXGNN_PICK_* of include/hexgnn.h


class ArenaResult:
    """One ``DeviceArena.play``: ``winner`` int8 [G] (0 = the maker player, 1 = the breaker player), ``length`` [G] (moves of
    the game, the opening included), ``moves`` [G][plies] vertex ids in the order played with -1 after a game's end, ``plies``
    the plies the batch took (its longest game).  Host arrays."""

    def __init__(self, winner, length, moves, plies):
        self.winner, self.length, self.moves, self.plies = winner, length, moves, plies

    @property
    def maker_wins(self) -> int:
        return int((self.winner == 0).sum())

    @property
    def breaker_wins(self) -> int:
        return int((self.winner == 1).sum())


def _is_random(player) -> bool:
    return isinstance(player, str) and player == "random"


def _is_search(player) -> bool:
    return hasattr(player, "search_scores")


def _observers(players):
    """Of ``((player, live_norm), ..)``: the players that follow the match (``begin_match()`` / ``observe_moves(moves)``, e.g.
    ``SearchPlayer(reuse_tree=True)``), each once even when it plays both sides."""
    out = []
    for p, _ in players:
        if hasattr(p, "begin_match") and hasattr(p, "observe_moves") and not any(p is o for o in out):
            out.append(p)
    return out


class DeviceArena:
    """``num_games`` games of Hex ``hex_size`` played in lock step on the device.  ``graph=True`` captures ``chunk`` plies (an
    even number, so that every chunk starts with the same side to move) as one HIP graph per (maker player, breaker player,
    first mover, pick mode, temperature); the models' weights are read at run time, so a cached graph follows training or
    ``load_state_dict``."""

    def __init__(self, hex_size: int, num_games: int, device=None, graph: bool = True, chunk: int = 8):
        if chunk < 2 or chunk % 2:
            raise ValueError("chunk must be a positive even number")
        if num_games < 1:
            raise ValueError("num_games must be positive")
        self.hex_size, self.num_games, self.chunk, self.use_graph = hex_size, num_games, chunk, bool(graph)
        self.mgr = mgr = Env_manager(num_games, hex_size, device=device)
        mgr.record_snapshots = False
        dev = self.device = mgr.device
        k, nv = num_games, mgr._nv
        e_max = int(mgr._base_sizes[0, 1])
        # capacity-sized observation (every env at the start position), as DeviceRollout keeps it; the players are not known
        # yet, so the tail clear is always there
        self.obs = ObsTarget.capacity(k, nv, e_max, dev, zeroed=True, tail_clear=True)
        off = np.zeros((2, k + 1), dtype=np.int32)
        off[0] = np.arange(k + 1) * nv
        off[1] = np.arange(k + 1) * e_max
        self._start_off = torch.from_numpy(off).to(dev)
        self.max_plies = hex_size * hex_size + chunk
        rows = -(-self.max_plies // chunk) * chunk
        self.log = torch.zeros((rows, k), dtype=torch.int32, device=dev)
        self.log_chunk = torch.zeros((chunk, k), dtype=torch.int32, device=dev)
        self.uni = torch.zeros((chunk, k), dtype=torch.float32, device=dev)
        self.result = torch.zeros((k, 5), dtype=torch.int32, device=dev)
        self.game = torch.zeros((k, 4), dtype=torch.int32, device=dev)
        self._game0 = torch.tensor([[-1, 0, 0, 0]], dtype=torch.int32, device=dev).repeat(k, 1)
        self.forced = torch.full((k,), -1, dtype=torch.int32, device=dev)
        self.live = torch.zeros(1, dtype=torch.int32, device=dev)
        self._graphs: Dict[tuple, tuple] = {}

    # -- pieces ----------------------------------------------------------------------------------------
    @staticmethod
    def _check_player(player):
        if _is_random(player) or _is_search(player):
            return False
        if not callable(player):
            raise TypeError("a player is a model from get_pre_defined or the string \"random\", not %r" % (player,))
        return live_norm_of(player)

    def _prepare(self, maker_first: bool, forced: Optional[torch.Tensor], players=()):
        """All envs at the start position with ``first`` to move, every game undecided, the openings in place; the players
        that follow the match (``_observers``) are told that one begins."""
        for p in _observers(players):
            p.begin_match()
        _lib.check(_lib.lib().hexgnn_env_reset(self.mgr._h, None, int(maker_first), None, ops._stream()), "hexgnn_env_reset")
        self.obs.node_off.copy_(self._start_off[0])
        self.obs.edge_off.copy_(self._start_off[1])
        self.game.copy_(self._game0)
        if forced is None:
            self.forced.fill_(-1)
        else:
            self.forced.copy_(forced)

    def _body(self, players, maker_first: bool, modes, temperature: float):
        """``chunk`` plies.  players / modes: (the maker's, the breaker's)."""
        L = _lib.lib()
        h, k, obs = self.mgr._h, self.num_games, self.obs
        maker = maker_first
        for t in range(self.chunk):
            obs.observe_env(h)
            (player, live_norm), mode = players[0 if maker else 1], modes[0 if maker else 1]
            q = None
            if _is_search(player):              # a tree search from the root env: the root visit counts are its scores
                active = ((self.game[:, 0] < 0) & (self.game[:, 3] == 0)).to(torch.int32)
                q = player.search_scores(h, obs, active)
            elif mode != PICK_UNIFORM:          # the built-in random player needs no forward
                q = acting_forward(player, obs, maker, self.mgr._nv, live_norm).reshape(-1)
                if q.dtype != torch.float32 or not q.is_contiguous():
                    q = q.float().contiguous()
            # a game that ends restarts on the side everyone moves to next
            _lib.check(L.hexgnn_arena_ply(h, obs.node_off.data_ptr(), q.data_ptr() if q is not None else None,
                                          obs.backmap.data_ptr(), mode, float(temperature) if mode == PICK_SOFTMAX else 1.0,
                                          self.uni[t].data_ptr(), self.forced.data_ptr(), int(not maker),
                                          self.game.data_ptr(), self.log_chunk[t].data_ptr(), self.result.data_ptr(),
                                          self.live.data_ptr(), ops._stream()), "hexgnn_arena_ply")
            _lib.check(L.hexgnn_env_offsets(k, self.result.data_ptr(), obs.node_off.data_ptr(), obs.edge_off.data_ptr(),
                                            ops._stream()), "hexgnn_env_offsets")
            for p in _observers(players):       # tree reuse: every such player sees its own move and the opponent's (-1: rests)
                p.observe_moves(self.log_chunk[t])
            maker = not maker

    # -- public ----------------------------------------------------------------------------------------
    def play(self, maker_player, breaker_player, first: str = "m", openings=None, temperature: float = 0.0,
             generator=None) -> ArenaResult:
        """One game per env between ``maker_player`` (always moves as maker, with its maker head) and ``breaker_player``;
        ``first`` ("m" / "b") moves at ply 0.  ``openings``: vertex ids (cell + 2), one per game, played at ply 0 instead of
        the first mover's choice.  ``temperature`` 0 is greedy, above 0 every model move is a draw from
        softmax(q / temperature) with uniforms from ``generator``; ``"random"`` draws uniformly over the legal moves."""
        if first not in ("m", "b"):
            raise ValueError("first must be \"m\" or \"b\"")
        temperature = float(temperature)
        if not temperature >= 0.0 or temperature == float("inf"):
            raise ValueError("temperature must be finite and >= 0")
        k = self.num_games
        if self.use_graph and (_is_search(maker_player) or _is_search(breaker_player)):
            raise ValueError("a search player reads sizes back inside a ply and cannot be captured: DeviceArena(graph=False)")
        players = tuple((p, self._check_player(p)) for p in (maker_player, breaker_player))
        modes = tuple(PICK_UNIFORM if _is_random(p) else (PICK_SOFTMAX if temperature > 0 else PICK_GREEDY)
                      for p in (maker_player, breaker_player))
        forced = None
        if openings is not None:
            forced = torch.as_tensor(np.asarray(openings, dtype=np.int32)).reshape(-1)
            if forced.numel() != k:
                raise ValueError("expected %d opening moves" % k)
            if int(forced.min()) < 2:
                raise ValueError("an opening move is a vertex id (board cell + 2)")
            forced = forced.to(self.device)
        maker_first = first == "m"
        needs_u = any(m != PICK_GREEDY for m in modes)
        step = None
        if self.use_graph:
            key = (id(maker_player), id(breaker_player), first, modes, temperature if PICK_SOFTMAX in modes else 0.0)
            ent = self._graphs.get(key)
            if ent is None:
                from .graphs import GraphedStep
                self._prepare(maker_first, None, players)        # the warm-up and the capture play real plies
                ent = (GraphedStep(lambda: self._body(players, maker_first, modes, temperature), warmup=1),
                       maker_player, breaker_player)    # keeps the models alive while their ids are a key
                self._graphs[key] = ent
            step = ent[0]
        self._prepare(maker_first, forced, players)
        plies, live = 0, k
        while live > 0:
            if plies >= self.max_plies:
                raise RuntimeError("%d games still undecided after %d plies of Hex-%d" % (live, plies, self.hex_size))
            if needs_u:
                for t in range(self.chunk):     # one draw per ply: the uniforms of a ply do not depend on the chunk length
                    torch.rand(k, generator=generator, out=self.uni[t])
            if step is not None:
                step.replay()
            else:
                self._body(players, maker_first, modes, temperature)
            self.log[plies:plies + self.chunk].copy_(self.log_chunk)
            plies += self.chunk
            live = int(self.live.item())                 # the one read-back per chunk
        game = self.game.cpu().numpy()
        moves = self.log[:plies].cpu().numpy().T.copy()
        if game[:, 3].any():
            g = int(np.nonzero(game[:, 3])[0][0])
            ply = int(game[g, 2])
            what = "illegal move %d" % int(moves[g, ply]) if game[g, 3] == 1 else "non-finite action values"
            raise ValueError("%s in game %d at ply %d" % (what, g, ply))
        used = int((moves >= 0).any(0).sum())
        return ArenaResult(game[:, 0].astype(np.int8), game[:, 1].astype(np.int64), moves[:, :used].astype(np.int64), used)


class Elo_handler:
    """Drop-in for ``Elo_handler`` of GN0/RainbowDQN/evaluate_elo.py:34-345 with the matches played by ``DeviceArena``.
    Players are models of ``gnn_hex_amd.models.get_pre_defined`` or the built-in random player (``add_player(name,
    model="random", simple=True)``); CNN, Gao-style and callable ``simple`` players and SGF logging raise
    ``NotImplementedError``."""

    def __init__(self, hex_size, empty_model_func=None, device="cuda", k=10):
        self.players = {}
        self.size = hex_size
        self.elo_league_contestants = list()
        self.device = device
        self.K = k
        self._arenas = {}
        if empty_model_func is not None:
            self.create_empty_models(empty_model_func)

    def reset(self, new_hex_size=None, keep_players=[]):
        self.players = {name: self.players[name] for name in keep_players if name in self.players}
        self.size = new_hex_size
        self._arenas = {}

    def create_empty_models(self, empty_model_func):
        self.empty_model1 = empty_model_func().to(self.device)
        self.empty_model1.eval()
        self.empty_model2 = empty_model_func().to(self.device)
        self.empty_model2.eval()

    def add_player(self, name, model=None, set_rating=None, simple=False, rating_fixed=False, episode_number=None,
                   checkpoint=None, can_join_roundrobin=True, uses_empty_model=True, cnn=False, cnn_hex_size=None,
                   gao_style=False, border_fill=True):
        self.players[name] = dict(model=model, simple=simple, rating=set_rating, rating_fixed=rating_fixed,
                                  episode_number=episode_number, checkpoint=checkpoint,
                                  can_join_roundrobin=can_join_roundrobin, uses_empty_model=uses_empty_model, cnn=cnn,
                                  cnn_hex_size=cnn_hex_size, gao_style=gao_style, border_fill=border_fill)

    # -- checkpoints -----------------------------------------------------------------------------------
    def load_into_empty_model(self, empty_model, checkpoint):
        stuff = torch.load(checkpoint, map_location=self.device, weights_only=False)
        empty_model.load_state_dict(stuff["state_dict"])
        if "cache" in stuff and stuff["cache"] is not None:
            empty_model.import_norm_cache(*stuff["cache"])

    def load_a_model_player(self, checkpoint, model_identifier, model_name=None, cnn_mode=False, cnn_hex_size=None,
                            gao_style=False, border_fill=True):
        from .models import get_pre_defined
        if model_name is None:
            model_name = os.path.basename(checkpoint)
        stuff = torch.load(checkpoint, map_location=self.device, weights_only=False)
        model = get_pre_defined(model_identifier, stuff["args"]).to(self.device)
        model.load_state_dict(stuff["state_dict"])
        self.add_player(name=model_name, model=model, simple=False, uses_empty_model=False, cnn=cnn_mode,
                        cnn_hex_size=cnn_hex_size, gao_style=gao_style, border_fill=border_fill)

    # -- matches ---------------------------------------------------------------------------------------
    def opening_moves(self) -> List[int]:
        """The unique opening moves as vertex ids: board cells i*n+i .. i*n+n-1 of the rows i = 0 .. n-1 (the others are
        their mirror images under the board's point symmetry), n (n + 1) / 2 of them; vertex id = cell + 2."""
        n = self.size
        return [i * n + j + 2 for i in range(n) for j in range(i, n)]

    def _player_for_arena(self, name):
        p = self.players[name]
        if p["cnn"] or p["gao_style"]:
            raise NotImplementedError("player %r: CNN / Gao-style players are outside the HIP path" % name)
        if p["simple"]:
            if _is_random(p["model"]):
                return "random"
            raise NotImplementedError("player %r: a simple player must be the built-in model=\"random\"; callables that "
                                      "walk Hex_game objects on the host are not supported" % name)
        if p["model"] is None:
            raise ValueError("player %r has no model (roundrobin loads checkpoints of uses_empty_model players)" % name)
        return p["model"]

    def _arena(self, games, graph: bool = True) -> DeviceArena:
        key = (self.size, games) if graph else (self.size, games, False)
        if key not in self._arenas:
            self._arenas[key] = DeviceArena(self.size, games, device=self.device, graph=graph)
        return self._arenas[key]

    def _match_plan(self, num_games, random_first_move):
        """(games per leg, their opening vertices): the shuffled unique openings, or uniformly random first moves."""
        starting_moves = self.opening_moves()
        random.shuffle(starting_moves)
        if num_games is None:
            num_games = 2 * len(starting_moves)
        if random_first_move:
            per_leg = num_games // 2
            n2 = self.size * self.size
            return per_leg, [[random.randrange(n2) + 2 for _ in range(per_leg)] for _ in range(2)]
        num_games = min(num_games, 2 * len(starting_moves))
        per_leg = num_games // 2
        return per_leg, [starting_moves[:per_leg], starting_moves[:per_leg]]

    def play_some_games(self, maker, breaker, num_games, temperature, random_first_move=False, progress=False,
                        log_sgfs=False):
        """A match of two legs of ``num_games // 2`` games, each one ``DeviceArena.play``: in leg 0 the maker player moves
        first, in leg 1 the breaker player.  Game i of a leg opens with the i-th of the shuffled unique opening moves
        (``random.shuffle``), so ``num_games`` is capped at n (n + 1) (``None`` = all).  ``random_first_move=True`` opens
        every game with a uniformly random cell instead and lifts the cap (the reference accepts the flag, but its branch
        is unreachable because its opening list is never None: it always plays the fixed openings).  ``temperature`` 0 is
        greedy.  Returns ``{maker: wins, breaker: wins}``."""
        if log_sgfs:
            raise NotImplementedError("SGF export is outside the HIP path")
        pm, pb = self._player_for_arena(maker), self._player_for_arena(breaker)
        per_leg, openings = self._match_plan(num_games, random_first_move)
        wins = {maker: 0, breaker: 0}
        lengths = []
        if per_leg > 0:
            arena = self._arena(per_leg, graph=not (_is_search(pm) or _is_search(pb)))     # a search player is not capturable
            for leg, first in enumerate(("m", "b")):
                res = arena.play(pm, pb, first=first, openings=openings[leg], temperature=temperature)
                wins[maker] += res.maker_wins
                wins[breaker] += res.breaker_wins
                lengths.extend(res.length.tolist())
        if progress and lengths:
            print("%s vs %s: %s, mean game length %.1f" % (maker, breaker, wins, float(np.mean(lengths))))
        return wins

    def roundrobin(self, num_players, num_games_per_match, must_include_players=[], score_as_n_games=20):
        ok_players = [x for x in self.players if self.players[x]["can_join_roundrobin"]]
        if num_players is None or num_players > len(ok_players):
            num_players = len(ok_players)
        contestants = list(must_include_players)
        while len(contestants) < num_players:
            name = random.choice(ok_players)
            if name not in contestants:
                contestants.append(name)
        all_stats = []
        for p1 in contestants:
            for p2 in contestants:
                if p1 == p2:
                    continue
                for name, empty in ((p1, "empty_model1"), (p2, "empty_model2")):
                    if self.players[name]["uses_empty_model"]:
                        self.players[name]["model"] = getattr(self, empty)
                        self.load_into_empty_model(self.players[name]["model"], self.players[name]["checkpoint"])
                all_stats.append(self.play_some_games(p1, p2, num_games_per_match, 0, random_first_move=False, progress=False))
        for _ in range(score_as_n_games):
            self.score_some_statistics(all_stats)
        performances = sorted(self.get_performances_from_stats(all_stats).items(), key=lambda x: -x[1])
        return ["name", "performance"], performances

    # -- ratings ---------------------------------------------------------------------------------------
    def get_rating(self, player_name):
        return self.players[player_name]["rating"]

    def _performance_sums(self, statistics, only_unrated):
        """Per player, over its statistics against rated opponents: sum(R_opp * games + 400 (2 wins - games)), sum(games)."""
        sums = defaultdict(lambda: [0.0, 0])
        for stats in statistics:
            a, b = list(stats.keys())
            games = int(stats[a]) + int(stats[b])
            for me, opp in ((a, b), (b, a)):
                if self.get_rating(opp) is None or (only_unrated and self.get_rating(me) is not None):
                    continue
                sums[me][0] += self.get_rating(opp) * games + 400 * (stats[me] * 2 - games)
                sums[me][1] += games
        return sums

    def get_performances_from_stats(self, statistics):
        return {name: num / games for name, (num, games) in self._performance_sums(statistics, False).items()}

    def score_some_statistics(self, statistics, game_num_independent=True):
        """One rating update from match statistics ``[{a: wins, b: wins}, ...]``, every term taken at the ratings before the
        call.  Rated players: R += K (score - expectation), per game when ``game_num_independent``, over their statistics
        against rated opponents, expectation = games / (1 + 10 ** ((R_opp - R_self) / 400)).  Players without a rating get
        their performance rating.  ``rating_fixed`` players never move."""
        acc = defaultdict(lambda: [0.0, 0.0, 0])         # expectation, score, games
        for stats in statistics:
            a, b = list(stats.keys())
            games = int(stats[a]) + int(stats[b])
            ra, rb = self.get_rating(a), self.get_rating(b)
            if ra is None or rb is None:
                continue
            for me, r_me, r_opp in ((a, ra, rb), (b, rb, ra)):
                acc[me][0] += (1 / (1 + 10 ** ((r_opp - r_me) / 400))) * games
                acc[me][1] += stats[me]
                acc[me][2] += games
        first = self._performance_sums(statistics, True)
        for name, (expectation, score, games) in acc.items():
            if not self.players[name]["rating_fixed"]:
                change = self.K * (score - expectation)
                if game_num_independent:
                    change /= games
                self.players[name]["rating"] += change
        for name, (num, games) in first.items():
            if not self.players[name]["rating_fixed"]:
                self.players[name]["rating"] = num / games

    def get_rating_table(self):
        data = [[name, self.get_rating(name)] for name in self.players if self.get_rating(name) is not None]
        data.sort(key=lambda x: -x[1])
        return ["name", "rating"], data
