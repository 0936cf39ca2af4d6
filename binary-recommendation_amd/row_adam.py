"""Adam state of the embedding tables of NeuMFEngine and BPREngine (and their row-sharded subclasses): Keras' non-lazy sparse Adam
[TF-sem] in one of three forms, fixed at construction.
  deferred ("adam_dense", dense_impl "deferred"): rows lag (last[k][row] = the last step a row includes) until a lookup replays the
           missed g = 0 steps, with the per-step scalars in the device step state.  Flushed before the alpha ring
           runs out (begin_steps) and before anything reads the tables (flush); all rows at step t after a load (_reset_lags).
  sweep    ("adam_dense", "sweep"): the touched rows, then one pass over every other row (mark[k] tells them apart).
  lazy     ("adam_lazy"): the touched rows only.
"""
from __future__ import annotations

import torch

from . import _lib, ops


class RowAdam:
    """Base class of the engines: they call _init_row_adam once their tables and moments exist."""

    ALPHA_RING = _lib.parse_enums()["BR_ALPHA_RING"]     # steps of alpha the device step state keeps for the replay
    step_state = None

    def _init_row_adam(self, tables: dict, optimizer: str, dense_impl: str, lr, beta1, beta2, eps, replay: str):
        """tables: stream ("user", "item") -> (table, m, v), the tensors the optimizer updates in place"""
        self.deferred = optimizer == "adam_dense" and dense_impl == "deferred"
        self._sweep = optimizer == "adam_dense" and not self.deferred
        self._rows, self._adam_hp, self._replay_form = tables, (lr, beta1, beta2, eps), replay
        self.t, self._flush_t, self._stale = 0, 0, False       # _stale: deferred rows lag behind self.t until flush()
        per_row = lambda dt: {k: torch.zeros(tab.shape[0], dtype=dt, device=tab.device) for k, (tab, _, _) in tables.items()}
        if self.deferred:
            self.last = per_row(torch.int32)
            self._step_state()
            self._set_step_state()
        elif self._sweep:
            self.mark = per_row(torch.uint8)                    # rows the step's row update touched: the sweep skips them

    def _step_state(self):
        """the device step state (include/binrec.h brStepStateBytes: step, alpha_t, alpha ring), made on first use"""
        if self.step_state is None:
            _, b1, b2, eps = self._adam_hp
            self.step_state = ops.new_step_state(self.device, b1, b2, eps, self._replay_form)
        return self.step_state

    def _set_step_state(self):
        """device step state := step self.t (if there is one)"""
        if self.step_state is not None:
            lr, b1, b2, _ = self._adam_hp
            _lib.check(_lib.load().brStepStateSet(self.step_state.data_ptr(), self.t, lr, b1, b2, ops._stream()), "brStepStateSet")

    def _advance_step_state(self, scratch=None):
        """the step body's launch that moves the device step counter and alpha ring one step on (and zeroes the float64 `scratch`)"""
        lr, b1, b2, _ = self._adam_hp
        _lib.check(_lib.load().brStepStateAdvance(self.step_state.data_ptr(), lr, b1, b2, None if scratch is None else scratch.data_ptr(),
                                                  0 if scratch is None else scratch.numel(), ops._stream()), "brStepStateAdvance")

    def begin_steps(self, n: int = 1):
        """before the next n steps' launches: flush while the alpha ring still holds every step a replay can need; then the rows lag"""
        if self.deferred:
            if self.t + n - self._flush_t >= self.ALPHA_RING - 8:
                self.flush()
            self._stale = True

    def flush(self):
        """deferred tables: apply every row's pending g = 0 steps (brAdamFlush), so that they hold step t.  A no-op otherwise."""
        if not (self.deferred and self._stale):
            return
        lib, (_, b1, b2, eps) = _lib.load(), self._adam_hp
        for k, (tab, m, v) in self._rows.items():
            _lib.check(lib.brAdamFlush(tab.data_ptr(), m.data_ptr(), v.data_ptr(), self.last[k].data_ptr(), tab.shape[0], tab.shape[1],
                                       self.step_state.data_ptr(), b1, b2, eps, ops._stream()), "brAdamFlush")
        self._stale, self._flush_t = False, self.t

    def _reset_lags(self):
        """after a checkpoint load (flushed tables): every row includes step t"""
        if self.deferred:
            for last in self.last.values():
                last.fill_(self.t)
            self._stale, self._flush_t = False, self.t
        self._set_step_state()

    def _row_tensors(self, k):
        return self._rows[k] + ((self.last[k],) if self.deferred else ())

    def _snapshot_rows(self, idx: dict):
        """stream -> int64 row ids: those rows of the table, its moments and `last` (what a dry-run step on them changes)"""
        return {k: (i, [t[i] for t in self._row_tensors(k)]) for k, i in idx.items()}

    def _restore_rows(self, snap):
        """write a _snapshot_rows back, in place"""
        for k, (i, rows) in snap.items():
            for t, r in zip(self._row_tensors(k), rows):
                t[i] = r

    def _adam_rows(self, k, index, g, ldg, g_hi=None, ldg_hi=0, split=0, replayed=None):
        """this step's Adam on the rows of table k that `index` names, row gradients g (g_hi: columns from `split` on) by index position.
        replayed (deferred): those rows as this step's lookup replayed them to step t-1 - the optimizer then replays the moments only."""
        tab, m, v = self._rows[k]
        lr, b1, b2, eps = self._adam_hp
        if self.deferred:
            ops.adam_rows_sorted_deferred(tab, m, v, self.last[k], index, g, ldg, self.step_state, b1, b2, eps, row_grads_hi=g_hi, ldg_hi=ldg_hi,
                                          split=split, replayed=replayed)
        else:
            ops.adam_rows_sorted(tab, m, v, index, g, ldg, ops.adam_alpha(lr, self.t, b1, b2), b1, b2, eps, mark=self.mark[k] if self._sweep else None,
                                 row_grads_hi=g_hi, ldg_hi=ldg_hi, split=split)

    def _adam_sweep(self, k):
        """sweep mode: this step's Adam on every row of table k that _adam_rows did not touch.  A no-op in the other modes."""
        if self._sweep:
            tab, m, v = self._rows[k]
            lr, b1, b2, eps = self._adam_hp
            ops.adam_dense_sweep(tab, m, v, ops.adam_alpha(lr, self.t, b1, b2), b1, b2, eps, mark=self.mark[k])

    def rows_as_of_previous_step(self, k, ids, out=None):
        """owner side of a lookup: rows `ids` of table k as this step reads them (deferred: replayed to step t-1 in registers)"""
        tab, m, v = self._rows[k]
        if self.deferred:
            _, b1, b2, eps = self._adam_hp
            return ops.gather_rows_deferred(tab, m, v, self.last[k], ids, self.step_state, b1, b2, eps, out=out, err_flag=self.err)
        return ops.gather_rows([tab], [ids], None if out is None else [out], err_flag=self.err)[0]
