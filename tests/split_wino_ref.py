"""A 3x3 layer (pad 1) on a 16 x 16 map in split Winograd form F(4x4,3x3), restated in float64 step by step as the device runs it
(kernels_level6.hip: split6_transform, level6_gemm over 36 positions, split6_inverse): the matrices, the tile order of
the rows, the channel padding and the weight order [position 6 r + q][output][input]."""
import torch

# points 0, +-1, +-2, inf (Lavin & Gray): the B^T, G and A^T of kernels_wino4.hip
BT = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]],
                  dtype=torch.float64)
G = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
                 dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=torch.float64)


def round_up(a, b):
    return (a + b - 1) // b * b


def rows(batch):
    """(R, bm): rows of a position and the GEMM's tile height (split6_rows)."""
    r = 16 * batch
    bm = 128 if r >= 1024 else 64 if r >= 512 else 32
    return round_up(r, bm), bm


def transform(x):
    """x [B, C, 16, 16] -> V [36][R][Kc]: B^T d B of the 6 x 6 window at (4 ty - 1, 4 tx - 1), row 16 b + 4 ty + tx, zero rows and channels."""
    B, C = x.shape[:2]
    R, _ = rows(B)
    Kc = round_up(C, 32)
    xp = torch.nn.functional.pad(x.double(), (1, 1, 1, 1))
    V = torch.zeros(36, R, Kc, dtype=torch.float64)
    for b in range(B):
        for ty in range(4):
            for tx in range(4):
                d = xp[b, :, 4 * ty:4 * ty + 6, 4 * tx:4 * tx + 6]            # [C, 6, 6]
                v = BT @ d @ BT.T                                               # [C, 6, 6]
                V[:, 16 * b + 4 * ty + tx, :C] = v.reshape(C, 36).T
    return V


def weights(w):
    """w [N, C, 3, 3] -> Wc [36][Npad][Kc]: (G g G^T)[r][q] at position 6 r + q, zero rows and columns."""
    N, C = w.shape[:2]
    Wc = torch.zeros(36, round_up(N, 128), round_up(C, 32), dtype=torch.float64)
    u = G @ w.double() @ G.T                                                    # [N, C, 6, 6]
    Wc[:, :N, :C] = u.reshape(N, C, 36).permute(2, 0, 1)
    return Wc


def gemm(V, Wc):
    """M'[xi][row][n] = sum_k V[xi][row][k] Wc[xi][n][k]"""
    return torch.einsum("xrk,xnk->xrn", V, Wc)


def inverse(Mp, batch, N, bias=None, relu=False):
    """M' [36][R][>= N] -> y [B, N, 16, 16]: A^T M' A per tile, + bias, ReLU."""
    y = torch.zeros(batch, N, 16, 16, dtype=torch.float64)
    for b in range(batch):
        for ty in range(4):
            for tx in range(4):
                m = Mp[:, 16 * b + 4 * ty + tx, :N].T.reshape(N, 6, 6)
                y[b, :, 4 * ty:4 * ty + 4, 4 * tx:4 * tx + 4] = AT @ m @ AT.T
    if bias is not None:
        y = y + bias.double().reshape(1, N, 1, 1)
    return y.clamp_min(0) if relu else y


def conv3x3(x, w, bias=None, relu=False):
    return inverse(gemm(transform(x), weights(w)), x.shape[0], w.shape[0], bias, relu)
