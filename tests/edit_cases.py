"""Case sets and the independent restatement of the edit-count rule shared by tests/test_edit_distance_cpu.py and
tests/test_gpu_edit_distance.py (not a test module).  Nothing here is imported from the package: ``rule`` is written from the text of
include/oasr.h with explicit (S, D, I) triples and a full table, no packing."""
import random

import torch

KNOWN = [([], [1, 2, 3], (0, 3, 0, 0)), ([1, 2, 3], [], (0, 0, 3, 0)), ([1, 9, 3], [1, 2, 3], (1, 0, 0, 2)), ([1, 3], [1, 2, 3], (0, 1, 0, 2)),
         ([1, 2, 2, 3], [1, 2, 3], (0, 0, 1, 3)), ([2, 1], [1, 2], (2, 0, 0, 0)), ([1, 1, 2], [1, 2], (0, 0, 1, 2)),
         ([0, 1, 0, 1], [1, 0, 1, 0], (0, 1, 1, 3))]
EDGE_LENGTHS = (0, 1, 63, 64, 65, 448, 1023)


def rule(hyp, ref):
    """(S, D, I, H) of one pair.  Cell (i, j) = (S, D, I) of hyp[:i] against ref[:j]; diagonal, then deletion, then insertion on a tie."""
    n, m = len(hyp), len(ref)
    prev = [(0, j, 0) for j in range(m + 1)]           # row 0: j deletions
    for i in range(1, n + 1):
        cur = [(0, 0, i)]                              # column 0: i insertions
        a = hyp[i - 1]
        for j in range(1, m + 1):
            dg, lf, up = prev[j - 1], cur[j - 1], prev[j]
            sub = 1 if a != ref[j - 1] else 0
            cd, cl, cu = dg[0] + dg[1] + dg[2] + sub, lf[0] + lf[1] + lf[2] + 1, up[0] + up[1] + up[2] + 1
            if cd <= cl and cd <= cu:
                cur.append((dg[0] + sub, dg[1], dg[2]))
            elif cl <= cu:
                cur.append((lf[0], lf[1] + 1, lf[2]))
            else:
                cur.append((up[0], up[1], up[2] + 1))
        prev = cur
    s, d, i = prev[m]
    return s, d, i, m - s - d


def binary_pairs():
    """Every pair of sequences over {0, 1} of length 0 .. 5: 63 x 63 = 3969."""
    seqs = [[(bits >> k) & 1 for k in range(n)] for n in range(6) for bits in range(1 << n)]
    return [(h, r) for h in seqs for r in seqs]


def random_pairs(n=300, seed=1234):
    """Seeded pairs of length 0 .. 40 over alphabets of 2, 3 and 50 symbols."""
    rng = random.Random(seed)
    out = []
    for t in range(n):
        a = (2, 3, 50)[t % 3]
        out.append(([rng.randrange(a) for _ in range(rng.randint(0, 40))], [rng.randrange(a) for _ in range(rng.randint(0, 40))]))
    return out


def length_pairs(lengths=EDGE_LENGTHS, seed=99):
    """One pair for every (hyp length, ref length) of ``lengths`` x ``lengths``, three symbols."""
    rng = random.Random(seed)
    return [([rng.randrange(3) for _ in range(n)], [rng.randrange(3) for _ in range(m)]) for n in lengths for m in lengths]


def pack(pairs, extra=0, fill=7):
    """Pairs -> (hyp int32 [B, Lh], hyp_len, ref int32 [B, Lr], ref_len) CPU tensors; the row widths are the longest lengths + ``extra`` and the
    cells past a length hold ``fill`` (tokens the operator must not read)."""
    B = len(pairs)
    Lh = max(len(h) for h, _ in pairs) + extra
    Lr = max(len(r) for _, r in pairs) + extra
    hyp, ref = torch.full((B, Lh), fill, dtype=torch.int32), torch.full((B, Lr), fill, dtype=torch.int32)
    for b, (h, r) in enumerate(pairs):
        hyp[b, :len(h)] = torch.tensor(h, dtype=torch.int32)
        ref[b, :len(r)] = torch.tensor(r, dtype=torch.int32)
    return (hyp, torch.tensor([len(h) for h, _ in pairs], dtype=torch.int32), ref, torch.tensor([len(r) for _, r in pairs], dtype=torch.int32))
