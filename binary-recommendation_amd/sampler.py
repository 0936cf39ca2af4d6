"""What the per-step samplers (bpr.NegativeSampler, neumf.BatchSampler) hold of a training set, built in one place."""
from __future__ import annotations

import torch

from . import ops


class CandidatePool:
    """The positives' CSR (ops.positives_csr), the candidate item ids (None: 0..n_items-1 with n_items = the largest positive item + 1)
    and, mode "popularity", Walker's alias table of count(item)^power over the given positives, restricted to the candidates."""

    def __init__(self, users, items, n_users: int, cand_items=None, mode: str = "uniform", power: float = 0.75, seed: int = 0, max_tries: int = 16,
                 device="cuda", n_items: int | None = None):
        import numpy as np
        if mode not in ("uniform", "popularity"):
            raise ValueError("mode must be 'uniform' or 'popularity'")
        if not 1 <= int(max_tries) <= 256:
            raise ValueError("max_tries must be in [1, 256]")
        self.mode, self.power, self.seed, self.max_tries = mode, float(power), int(seed), int(max_tries)
        self.device = torch.device(device)
        self.pos_off, self.pos_items = ops.positives_csr(users, items, int(n_users), self.device)
        it = np.asarray(items.cpu() if torch.is_tensor(items) else items).astype(np.int64)
        if cand_items is None:
            self.cand_items = None
            self.n_cand = int(n_items) if n_items is not None else int(it.max()) + 1
            cand = np.arange(self.n_cand, dtype=np.int64)
        else:
            cand = np.asarray(cand_items.cpu() if torch.is_tensor(cand_items) else cand_items).astype(np.int64)
            self.cand_items = torch.from_numpy(cand).to(self.device).to(self.pos_items.dtype).contiguous()
            self.n_cand = int(cand.shape[0])
        self.alias = None
        if mode == "popularity":
            count = np.bincount(it, minlength=int(max(it.max(), cand.max())) + 1).astype(np.float64)
            self.alias = ops.alias_table(count[cand] ** self.power, device=self.device)
