"""Host-side helpers for the batched RD entry (svt_hip_rd_batch): job / quantizer-row construction and a
torch-backed runner.  torch is plumbing here (device buffers on the context's stream); the compute is in libsvthip.so."""
import ctypes as C

import numpy as np

from . import abi, api


def quant_row_from_step(dc_step, ac_step):
    """A plausible SvtHipQuantRow for dequantizer steps (dc, ac), built the way libaom's av1_build_quantizer fills
    its rows (invert_quant, zbin = 84/128 step, round = 48/128 step, fp round = 64/128 step).  Synthetic stand-in for
    the encoder's per-qindex tables, which the real caller passes in (Codec/full_loop.c:1627-1685)."""
    row = np.zeros((), dtype=abi.QUANT_ROW_DTYPE)
    for i, d in enumerate((int(dc_step), int(ac_step))):
        # invert_quant(): t = 1 + (1 << 16) * ((1 << l) - d) / d, shift = 1 << (16 - l), l = floor(log2(d))
        l = d.bit_length() - 1
        m = 1 + (1 << (16 + l)) // d
        row["quant"][i] = np.array(m - (1 << 16), np.int64).astype(np.int16)  # (int16_t) cast, wraps like the C code
        row["quant_shift"][i] = np.array(1 << (16 - l), np.int64).astype(np.int16)
        row["zbin"][i] = (84 * d + 64) >> 7
        row["round"][i] = (48 * d) >> 7
        row["quant_fp"][i] = min((1 << 16) // d, 32767)
        row["round_fp"][i] = (64 * d) >> 7
        row["dequant"][i] = d
    return row


def grid_jobs(width, height, stride, tx_size, tx_type=0, quant_row=0, org=0):
    """One job per tx block tiling a width x height picture (offsets in samples, row-major)."""
    w, h = abi.TX_W[tx_size], abi.TX_H[tx_size]
    ys, xs = np.meshgrid(np.arange(0, height - h + 1, h), np.arange(0, width - w + 1, w), indexing="ij")
    jobs = np.zeros(ys.size, dtype=abi.JOB_DTYPE)
    jobs["src_offset"] = (org + ys.ravel() * stride + xs.ravel()).astype(np.uint32)
    jobs["pred_offset"] = jobs["src_offset"]
    jobs["tx_type"] = tx_type
    jobs["quant_row"] = quant_row
    return jobs


OPTIONAL_OUTPUTS = ("coeff", "qcoeff", "dqcoeff", "cul_level", "recon")  # eob .. sse are mandatory


class Enqueued:
    """An RD batch on the context stream: `outs` = the per-job output arrays as device byte tensors by name, `recon` = the recon plane's tensor
    or None.  The object also holds the uploaded inputs, so keep it until the stream has run."""

    def __init__(self, outs, shapes, recon, slots, inputs):
        self.outs, self.shapes, self.recon, self.slots, self._inputs = outs, shapes, recon, slots, inputs

    def download(self):
        """the per-job outputs as numpy arrays [slots, elements per job] (after ctx.sync())"""
        return {name: api.to_host(self.outs[name], dt, (self.slots, k)) for name, (dt, k) in self.shapes.items()}


def enqueue_hip(ctx, desc_fields, src, pred, jobs, quant_rows, want_coeffs=True, want_recon=True, qmatrix=None, iqmatrix=None, outputs=None,
                spare_jobs=0, fill=0, recon_init=None):
    """Uploads the inputs and enqueues svt_hip_rd_batch on the context stream without waiting for it: returns an Enqueued, whose `outs` stay
    on the device for a following batch on the same stream (rate.run_rate_device reads outs["qcoeff"] / outs["eob"] / outs["dist_coeff"] in
    place).  Arguments as run_hip's."""
    import torch
    if outputs is None:
        outputs = ("cul_level",) + (("coeff", "qcoeff", "dqcoeff") if want_coeffs else ()) + (("recon",) if want_recon else ())
    unknown = set(outputs) - set(OPTIONAL_OUTPUTS)
    if unknown:
        raise ValueError(f"unknown RD outputs {sorted(unknown)}")
    ts = desc_fields["tx_size"]
    npk = min(abi.TX_W[ts], 32) * min(abi.TX_H[ts], 32)
    n = len(jobs)
    slots = n + spare_jobs
    t_src, t_pred, t_jobs, t_q = (api.to_device(a) for a in (src, pred, jobs, quant_rows))
    shapes = {name: (np.dtype(dt), k) for name, dt, k in abi.RD_OUT_FIELDS if name != "cul_level" or name in outputs}
    shapes.update({name: (np.dtype(np.int32), npk) for name in ("coeff", "qcoeff", "dqcoeff") if name in outputs})
    outs = {name: torch.full((slots * k * dt.itemsize,), fill, dtype=torch.uint8, device="cuda") for name, (dt, k) in shapes.items()}
    want_recon = "recon" in outputs
    t_rec = (t_pred.clone() if recon_init is None else api.to_device(np.asarray(recon_init, pred.dtype).reshape(pred.shape))) if want_recon else None
    d = abi.RdBatchDesc(n_jobs=n, src=t_src.data_ptr(), pred=t_pred.data_ptr(), recon=t_rec.data_ptr() if want_recon else None,
                        jobs=t_jobs.data_ptr(), quant_rows=t_q.data_ptr(), n_quant_rows=len(quant_rows), **desc_fields)
    for name, t in outs.items():
        setattr(d, name, t.data_ptr())
    keep = [t_src, t_pred, t_jobs, t_q]
    if qmatrix is not None:
        t_qm, t_iqm = api.to_device(qmatrix, np.uint8), api.to_device(iqmatrix, np.uint8)
        d.qmatrix, d.iqmatrix = t_qm.data_ptr(), t_iqm.data_ptr()
        keep += [t_qm, t_iqm]
    torch.cuda.synchronize()
    ctx.check(api.lib().svt_hip_rd_batch(ctx._h, C.byref(d)), "svt_hip_rd_batch")
    return Enqueued(outs, shapes, t_rec, len(jobs) + spare_jobs, keep)


def run_hip(ctx, desc_fields, src, pred, jobs, quant_rows, want_coeffs=True, want_recon=True, qmatrix=None, iqmatrix=None, outputs=None,
            spare_jobs=0, fill=0, recon_init=None):
    """Runs svt_hip_rd_batch on device copies of the inputs; returns numpy results.
    outputs: the optional outputs to request, a subset of OPTIONAL_OUTPUTS; None = cul_level plus what want_coeffs / want_recon select.
    Every per-job output array gets `spare_jobs` slots past n_jobs; all of them start as the byte `fill` and come back whole.
    recon_init: the recon plane's content before the call (same shape and dtype as pred); None = a copy of pred."""
    run = enqueue_hip(ctx, desc_fields, src, pred, jobs, quant_rows, want_coeffs, want_recon, qmatrix, iqmatrix, outputs, spare_jobs, fill, recon_init)
    ctx.sync()
    res = run.download()
    if run.recon is not None:
        res["recon"] = api.to_host(run.recon, pred.dtype, pred.shape)
    return res


def run_fwd_hip(ctx, tx_size, residual, jobs, spare_jobs=0, fill=0):
    """Runs svt_hip_fwd_txfm_batch on a device copy of the int16 residual plane (2-D, row stride = its width); returns the int32
    coefficients [n_jobs + spare_jobs, W * H], every slot starting as the byte `fill`."""
    import torch
    residual = np.ascontiguousarray(residual, np.int16)
    n, wh = len(jobs), abi.TX_W[tx_size] * abi.TX_H[tx_size]
    t_res, t_jobs = api.to_device(residual), api.to_device(jobs)
    t_co = torch.full(((n + spare_jobs) * wh * 4,), fill, dtype=torch.uint8, device="cuda")
    d = abi.FwdTxBatchDesc(tx_size=tx_size, n_jobs=n, residual_stride=residual.shape[1], residual=t_res.data_ptr(), jobs=t_jobs.data_ptr(),
                           coeff=t_co.data_ptr())
    torch.cuda.synchronize()
    ctx.check(api.lib().svt_hip_fwd_txfm_batch(ctx._h, C.byref(d)), "svt_hip_fwd_txfm_batch")
    ctx.sync()
    return api.to_host(t_co, np.int32, (n + spare_jobs, wh))


def run_inv_hip(ctx, bit_depth, tx_size, pred, jobs, dqcoeff, recon=None):
    """Runs svt_hip_inv_txfm_batch: pred and recon are 2-D planes of the same dtype (uint8: 8-bit only; uint16), each with its
    own row stride; recon = None runs in place (the recon plane IS the prediction plane).  Returns the recon plane."""
    import torch
    pred = np.ascontiguousarray(pred)
    t_pred, t_co, t_jobs = api.to_device(pred), api.to_device(dqcoeff, np.int32), api.to_device(jobs)
    out = pred if recon is None else np.ascontiguousarray(recon, pred.dtype)
    t_rec = t_pred if recon is None else api.to_device(out)
    d = abi.InvTxBatchDesc(bit_depth=bit_depth, sample_bytes=pred.dtype.itemsize, tx_size=tx_size, n_jobs=len(jobs), pred_stride=pred.shape[1],
                           recon_stride=out.shape[1], pred=t_pred.data_ptr(), recon=t_rec.data_ptr(), jobs=t_jobs.data_ptr(), dqcoeff=t_co.data_ptr())
    torch.cuda.synchronize()
    ctx.check(api.lib().svt_hip_inv_txfm_batch(ctx._h, C.byref(d)), "svt_hip_inv_txfm_batch")
    ctx.sync()
    return api.to_host(t_rec, pred.dtype, out.shape)
