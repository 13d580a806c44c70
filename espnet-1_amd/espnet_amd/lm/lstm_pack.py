"""The packed weight operands of the LSTM kernels (ea_lstm_step, ea_lstm_cell_fwd,
ea_lstm_cell_bwd): the slice-major tile layout of include/espnet_amd.h ("LSTM weight packs").

Every pack is made the same way: the weights are laid into a zero-padded f32 staging matrix
(tiles * 16 rows, K) whose rows stand in tile order, and one strided copy between tile_views'
views writes the flat operand.  The forward tiles hold 4 hidden units x 4 gates (gate_rows),
the backward tiles 16 hidden units of weight_hh^T.
"""
import torch

from .._lib import LSTM_KG

KG = LSTM_KG  # K granule of the packed operands
TILE_UNITS = 4  # hidden units per forward tile (x 4 gates = 16 rows, one MFMA column tile)


def rup(x: int, g: int = KG) -> int:
    return (x + g - 1) // g * g


def tile_views(stage: torch.Tensor, out: torch.Tensor):
    """stage (tiles * 16, K) f32, out flat with as many elements -> (src, dst) such that
    dst.copy_(src) writes element (tile t, slice s, row r, j) = stage[16 * t + r, s * SL + j] at
    out[((t * nks + s) * 16 + r) * SL + j], rounded to out's dtype.  SL, the K depth of one
    slice, is one 16-B load per lane: 16 (f32) or 32 (bf16)."""
    SL = 32 if out.dtype == torch.bfloat16 else 16
    rows, K = stage.shape
    return stage.view(rows // 16, 16, K // SL, SL).permute(0, 2, 1, 3), out.view(rows // 16, K // SL, 16, SL)


def gate_rows(stage: torch.Tensor) -> torch.Tensor:
    """The (gate, unit, k) view of a forward staging matrix: its row 16 * t + 4 * u + gate is
    gate `gate` (torch order i, f, g, o) of hidden unit 4 * t + u."""
    return stage.view(-1, 4, stage.shape[1]).permute(1, 0, 2)


def pack_lstm_weights(w_ih: torch.Tensor, w_hh: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """(4H, I), (4H, H) torch LSTM weights -> the operand of ea_lstm_step: forward tiles of
    [W_ih | 0 | W_hh | 0], K = Ip + Hp."""
    H, I = w_hh.shape[1], w_ih.shape[1]
    if w_ih.shape[0] != 4 * H or w_hh.shape[0] != 4 * H:
        raise ValueError(f"not LSTM weights: {tuple(w_ih.shape)}, {tuple(w_hh.shape)}")
    Ip, Hp = rup(I), rup(H)
    stage = torch.zeros(rup(H, TILE_UNITS) * 4, Ip + Hp, dtype=torch.float32, device=w_ih.device)
    rows = gate_rows(stage)
    rows[:, :H, :I] = w_ih.detach().float().view(4, H, I)
    rows[:, :H, Ip:Ip + H] = w_hh.detach().float().view(4, H, H)
    out = torch.empty(stage.numel(), dtype=dtype, device=stage.device)
    src, dst = tile_views(stage, out)
    return dst.copy_(src).view(-1)


def pack_lstm_bias(b_ih: torch.Tensor, b_hh: torch.Tensor) -> torch.Tensor:
    """(4H,) + (4H,) -> f32 (4H,) with [4 * unit + gate] = b_ih + b_hh of row gate * H + unit."""
    out = torch.empty(b_ih.numel(), 1, dtype=torch.float32, device=b_ih.device)
    gate_rows(out)[:, :, 0] = (b_ih.detach().float() + b_hh.detach().float()).view(4, -1)
    return out.view(-1)


class HHPacks:
    """Both packs of one layer's weight_hh, the operands of ea_lstm_cell_fwd (fwd: forward tiles,
    K = Hp) and ea_lstm_cell_bwd (bwd: weight_hh^T in tiles of 16 hidden units, K = 4H padded),
    with their staging matrices, so that refresh() is four strided copies on the current stream:
    no allocation, no host synchronisation (it runs after every optimizer step)."""

    def __init__(self, w_hh: torch.Tensor, dtype):
        G, H = w_hh.shape
        if G != 4 * H:
            raise ValueError(f"not an LSTM weight_hh: {tuple(w_hh.shape)}")
        self.H, self.dtype = H, dtype
        self._stage = torch.zeros(rup(H, TILE_UNITS) * 4, rup(H), dtype=torch.float32, device=w_hh.device)
        self._stage_t = torch.zeros(rup(H, 16), rup(G), dtype=torch.float32, device=w_hh.device)
        self.fwd = torch.zeros(self._stage.numel(), dtype=dtype, device=w_hh.device)
        self.bwd = torch.zeros(self._stage_t.numel(), dtype=dtype, device=w_hh.device)
        self._rows, self._rows_t = gate_rows(self._stage)[:, :H, :H], self._stage_t[:H, :G]
        self._src, self._dst = tile_views(self._stage, self.fwd)
        self._src_t, self._dst_t = tile_views(self._stage_t, self.bwd)

    @torch.no_grad()
    def refresh(self, w_hh: torch.Tensor):
        self._rows.copy_(w_hh.detach().view(4, self.H, self.H))
        self._dst.copy_(self._src)
        self._rows_t.copy_(w_hh.detach().t())
        self._dst_t.copy_(self._src_t)
        return self


def pack_lstm_hh(w_hh: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """(4H, H) torch weight_hh -> the operand of ea_lstm_cell_fwd (a fresh HHPacks' fwd)."""
    return HHPacks(w_hh, dtype).refresh(w_hh).fwd


def pack_lstm_hh_t(w_hh: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """(4H, H) torch weight_hh -> the operand of ea_lstm_cell_bwd (a fresh HHPacks' bwd)."""
    return HHPacks(w_hh, dtype).refresh(w_hh).bwd
