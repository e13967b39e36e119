"""Decoder level 6 with the transposed conv composed into the first 3x3 conv, restated in float64 torch: the specification that
ccvpe_amd/csrc/kernels_level6.hip and ensure_level6 (ccvpe_weights.hip) follow, step by step.

    x[B,K,8,8] -> deconv (k2 s2, K -> Cd) -> cat [Cd | skip Cs] -> conv 3x3 (Cd + Cs -> N) -> ReLU

Per output parity class (py, px) the Cd-channel half is a 2x2-tap convolution K -> N on the 8x8 grid, run as Winograd F(MxM,2x2),
M = 4 (25 positions) or 2 (9 positions).  Tensors are NCHW here; the library keeps NHWC."""
import torch

F64 = torch.float64

# Cook-Toom matrices of y[i] = sum_k d[i + k] g[k], i < M, k < 2:  y = A^T [(G g) * (B^T d)]
MATRICES = {
    4: dict(  # points 0, 1, -1, 2, inf
        BT=[[2, -1, -2, 1, 0], [0, -2, -1, 1, 0], [0, 2, -3, 1, 0], [0, -1, 0, 1, 0], [0, 2, -1, -2, 1]],
        AT=[[1, 1, 1, 1, 0], [0, 1, -1, 2, 0], [0, 1, 1, 4, 0], [0, 1, -1, 8, 1]],
        G=[[1 / 2, 0], [-1 / 2, -1 / 2], [-1 / 6, 1 / 6], [1 / 6, 1 / 3], [0, 1]]),
    2: dict(  # points 0, 1, inf
        BT=[[-1, 1, 0], [0, 1, 0], [0, -1, 1]],
        AT=[[1, 1, 0], [0, 1, 1]],
        G=[[-1, 0], [1, 1], [0, 1]]),
}


def matrices(m):
    return {k: torch.tensor(v, dtype=F64) for k, v in MATRICES[m].items()}


def compose_weights(wd, bd, wa, ba):
    """Step 1a.  wd [K, Cd, 2, 2], bd [Cd]: the transposed conv; wa [N, Cd + Cs, 3, 3], ba [N]: the conv.
    Returns w2 [2, 2, 2, 2, K, N] indexed [py][px][a][b] and bc [9, N] (3 * row case + column case; 0 interior, 1 first, 2 last).

    Conv pixel (2I + py, 2J + px), tap (ky, kx) reads transposed-conv pixel (2I + py + ky - 1, ...) = input pixel
    (I - 1 + py + a, J - 1 + px + b) at parity (ty & 1, tx & 1), ty = py + ky + 1, a = (ty >> 1) - py (likewise for x)."""
    wd, bd, wa, ba = wd.to(F64), bd.to(F64), wa.to(F64), ba.to(F64)
    K, Cd = wd.shape[:2]
    N = wa.shape[0]
    w2 = torch.zeros(2, 2, 2, 2, K, N, dtype=F64)
    for py in range(2):
        for px in range(2):
            for ky in range(3):
                for kx in range(3):
                    ty, tx = py + ky + 1, px + kx + 1
                    a, b = (ty >> 1) - py, (tx >> 1) - px
                    w2[py, px, a, b] += wd[:, :, ty & 1, tx & 1] @ wa[:, :Cd, ky, kx].T
    bc = torch.zeros(9, N, dtype=F64)
    for rcase in range(3):
        for ccase in range(3):
            acc = ba.clone()
            for ky in range(3):
                for kx in range(3):
                    if (rcase == 1 and ky == 0) or (rcase == 2 and ky == 2) or (ccase == 1 and kx == 0) or (ccase == 2 and kx == 2):
                        continue
                    acc += wa[:, :Cd, ky, kx] @ bd
            bc[rcase * 3 + ccase] = acc
    return w2, bc


def filter_transform(w2, m):
    """Step 1b.  [2, 2, 2, 2, K, N] -> u [4 classes, NP, NP, K, N]: G w G^T per class, channel pair."""
    G = matrices(m)["G"]
    return torch.einsum("ua,vb,pqabkn->pquvkn", G, G, w2).reshape(4, G.shape[0], G.shape[0], *w2.shape[4:])


def input_transform(x, m):
    """Step 2.  x [B, K, 8, 8] -> v [4 classes, NP, NP, B * T * T rows, K]: the window of class (py, px), tile (ty, tx) starts at
    (m ty - 1 + py, m tx - 1 + px); zeros outside the grid."""
    BT = matrices(m)["BT"]
    B, K = x.shape[:2]
    T, NP = 8 // m, m + 1
    xp = torch.zeros(B, K, 8 + 2 * m, 8 + 2 * m, dtype=F64)   # (margin m: every window fits)
    xp[:, :, m:m + 8, m:m + 8] = x.to(F64)
    v = torch.zeros(4, NP, NP, B * T * T, K, dtype=F64)
    for py in range(2):
        for px in range(2):
            for b in range(B):
                for ty in range(T):
                    for tx in range(T):
                        y0, x0 = m * ty - 1 + py + m, m * tx - 1 + px + m
                        d = xp[b, :, y0:y0 + NP, x0:x0 + NP]                       # [K, NP, NP]
                        v[py * 2 + px, :, :, (b * T + ty) * T + tx] = torch.einsum("ui,vj,kij->uvk", BT, BT, d)
    return v


def grouped_gemm(v, u):
    """Step 3.  [4, NP, NP, rows, K] x [4, NP, NP, K, N] -> [4, NP, NP, rows, N]."""
    return torch.einsum("cuvrk,cuvkn->cuvrn", v, u)


def skip_half(skip, wa, cd):
    """Step 4.  The conv over the skip channels alone: no bias, no activation."""
    return torch.nn.functional.conv2d(skip.to(F64), wa.to(F64)[:, cd:], None, padding=1)


def combine(mp, sk, bc, m, batch):
    """Step 5.  A^T M' A per (class, tile, channel), + skip half, + bc[border case], ReLU -> [B, N, 16, 16]."""
    AT = matrices(m)["AT"]
    T = 8 // m
    N = mp.shape[-1]
    out = torch.zeros(batch, N, 16, 16, dtype=F64)
    for py in range(2):
        for px in range(2):
            y = torch.einsum("iu,jv,uvrn->rnij", AT, AT, mp[py * 2 + px])      # [rows, N, m, m]
            for b in range(batch):
                for ty in range(T):
                    for tx in range(T):
                        r = (b * T + ty) * T + tx
                        out[b, :, 2 * m * ty + py:2 * m * (ty + 1):2, 2 * m * tx + px:2 * m * (tx + 1):2] = y[r]
    case = torch.zeros(16, dtype=torch.long)
    case[0], case[15] = 1, 2
    idx = case[:, None] * 3 + case[None, :]                                     # [16, 16]
    out = out + sk + bc[idx].permute(2, 0, 1)[None]
    return torch.relu(out)


def level6_composed(x, skip, wd, bd, wa, ba, m=4):
    w2, bc = compose_weights(wd, bd, wa, ba)
    mp = grouped_gemm(input_transform(x, m), filter_transform(w2, m))
    return combine(mp, skip_half(skip, wa, wd.shape[1]), bc, m, x.shape[0])


def level6_direct(x, skip, wd, bd, wa, ba):
    f = torch.nn.functional
    up = f.conv_transpose2d(x.to(F64), wd.to(F64), bd.to(F64), stride=2)
    return torch.relu(f.conv2d(torch.cat([up, skip.to(F64)], 1), wa.to(F64), ba.to(F64), padding=1))
