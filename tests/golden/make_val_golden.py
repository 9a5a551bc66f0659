"""Fixture for LitGINI.validation_step's arithmetic: ``val_step.npz``.

Runs the reference's OWN ``calculate_top_k_prec`` / ``calculate_top_k_recall``
(deepinteract_utils.py:977-995) and the validation step's own index line
(deepinteract_modules.py:1928, ``examples[:, 1] + logits.shape[2] * examples[:, 0]`` on the squeezed
[2, L1, L2] logits) on a few seeded pools of sampled example rows, through ``refshim`` as
``make_golden.py`` does. A pool is what the step concatenates over the complexes of one batch.

Every pool's scores are distinct, so the reference's ``argsort`` has one answer and the fixture is
exact. Where the reference raises ZeroDivisionError (k = 0, or no positive label) the figure is
stored as NaN. The pools:

  a  one complex, k = l = N
  b  k > N for every k but l // 5, and l // 10 = 0
  c  two complexes pooled, rows repeated within and across the complexes' lists
  d  no positive label
  e  a larger pool: N = 300 of 30 x 40 pairs, l = 70

Per pool p: ``p_l``, ``p_scores`` [N] fp32 (the class-1 probabilities), ``p_labels`` [N] int64,
``p_figures`` [6] fp64 (top_10_prec, top_l_by_10_prec, top_l_by_5_prec, top_l_recall,
top_l_by_2_recall, top_l_by_5_recall), and per complex c of it ``p_c_examples`` [n, 3] int64,
``p_c_shape`` (L1, L2), ``p_c_index`` [n] (the index line's result).

Usage (build container only; the fixture is committed):  python tests/golden/make_val_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import refshim  # noqa: E402

# name: (l, positive rate, [(L1, L2, rows, rows repeated from the pool so far)])
POOLS = {
    "a": (12, 0.3, [(5, 7, 12, 0)]),
    "b": (7, 0.5, [(3, 4, 6, 0)]),
    "c": (24, 0.25, [(6, 5, 20, 4), (4, 9, 15, 5)]),
    "d": (8, 0.0, [(4, 4, 10, 0)]),
    "e": (70, 0.1, [(30, 40, 300, 0)]),
}


def main():
    _, du = refshim.reference_modules()
    out = {"pools": np.array(sorted(POOLS))}
    for seed, name in enumerate(sorted(POOLS)):
        l, rate, complexes = POOLS[name]
        g = torch.Generator().manual_seed(100 + seed)
        lists = []
        for c, (l1, l2, rows, repeats) in enumerate(complexes):
            flat = torch.randperm(l1 * l2, generator=g)[:rows - repeats]
            flat = torch.cat((flat, flat[torch.randint(0, flat.numel(), (repeats,), generator=g)]))
            flat = flat[torch.randperm(rows, generator=g)]
            lab = (torch.rand(rows, generator=g) < rate).long()
            examples = torch.stack((flat // l2, flat % l2, lab), dim=1)
            logits = torch.zeros(2, l1, l2)                       # the step's squeezed logits: shape only
            index = examples[:, :2][:, 1] + logits.shape[2] * examples[:, :2][:, 0]
            out[f"{name}_{c}_examples"], out[f"{name}_{c}_index"] = examples.numpy(), index.numpy()
            out[f"{name}_{c}_shape"] = np.array([l1, l2])
            lists.append(examples)
        labels = torch.cat(lists)[:, 2]
        n = labels.numel()
        scores = ((torch.randperm(n, generator=g).float() + 0.5) / n)          # distinct: no ties
        order = torch.argsort(scores, descending=True)
        figures = []
        for fn, k in ((du.calculate_top_k_prec, 10), (du.calculate_top_k_prec, l // 10),
                      (du.calculate_top_k_prec, l // 5), (du.calculate_top_k_recall, l),
                      (du.calculate_top_k_recall, l // 2), (du.calculate_top_k_recall, l // 5)):
            try:
                figures.append(float(fn(order, labels, k=k)))
            except ZeroDivisionError:
                figures.append(float("nan"))
        out[f"{name}_l"], out[f"{name}_scores"], out[f"{name}_labels"] = np.array(l), scores.numpy(), labels.numpy()
        out[f"{name}_figures"] = np.array(figures, dtype=np.float64)
        assert len(set(scores.tolist())) == n
        print(name, "N", n, "l", l, "positives", int(labels.sum()), figures)
    path = os.path.join(HERE, "val_step.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
