"""torch.autograd wrappers of the device simulators: `abr` and `abr2` run mbfir.abr_batch / mbfir.abr2_batch on one pulse and are
differentiable in rf, their backward being one mbfir.abr_vjp_batch / mbfir.abr2_vjp_batch call and their
forward-mode tangent one mbfir.abr_jvp_batch / mbfir.abr2_jvp_batch call with one direction (section 8l), so that
torch.autograd.forward_ad dual tensors and torch.func.jvp pass through them.  They are also differentiable, in reverse mode, in the
gradient waveform g when g is a tensor that requires grad (float64 in 1D, complex128 in 2D): the backward is then one
mbfir.abr_vjp_rfg_batch / mbfir.abr2_vjp_rfg_batch call that returns both gradients (section 8o); when only rf requires grad it is
the rf call, with its bits.  A forward-mode tangent for g raises NotImplementedError.  rf is a complex128 tensor; the C ABI takes
host pointers, so tensors go through host memory, and the results come back on rf's device.
x, y and the scales are constants of the graph.  torch is imported on first use, not with the package.
`bloch` runs mbfir.bloch_batch on one pulse (the Bloch simulation with T1 / T2, end point) and is differentiable in reverse mode in
b1 and in the initial magnetisation m0, its backward being one mbfir.bloch_vjp_batch call (section 8p); with forward_mode=True it
also has the forward-mode tangent in both, one mbfir.bloch_jvp_batch call with one direction (section 8q).  It is also
differentiable, in reverse mode, in the gradient waveform gr and in the off-resonance df when they are float64 tensors that require
grad: the backward is then one mbfir.bloch_vjp_gr_batch call for every gradient that is wanted (section 8w); when neither does it is
the b1 call, with its bits.  A forward-mode tangent for gr or df raises NotImplementedError.  With steady_state=True
it returns the steady state of the period instead (bloch_batch mode 1), differentiable in b1 through mbfir.bloch_ss_vjp_batch and
mbfir.bloch_ss_jvp_batch (section 8t) and, in reverse mode, in gr and df through mbfir.bloch_ss_vjp_gr_batch (section 8x).
`bloch_train` runs mbfir.bloch_train_batch on one period (the echo-by-echo transient of a pulse train) and is differentiable in
reverse mode in b1 and in m0, its backward being one mbfir.bloch_train_vjp_batch call (section 8z); with forward_mode=True it also
has the forward-mode tangent in both, one mbfir.bloch_train_jvp_batch call with one direction (section 8aa).  Its gains and phases
may be float64 tensors of shape (ntr,) that require grad: the backward then has one mbfir.bloch_train_vjp_sched_batch call for the
schedule's per-repetition gradients (section 8ad); with forward_mode=True the schedule has its forward-mode tangent as well, one
mbfir.bloch_train_jvp_sched_batch call with one direction (section 8ae), and without it such a tangent raises NotImplementedError.
Its gr and df may be float64 tensors that require grad as `bloch`'s may: the backward is then one mbfir.bloch_train_vjp_gr_batch
call for every gradient that is wanted (section 8aj); a forward-mode tangent for either raises NotImplementedError.

    rf = torch.tensor(rf0, dtype=torch.complex128, requires_grad=True)
    g = torch.tensor(g0, dtype=torch.complex128, requires_grad=True)       # or an array: a constant
    a, b = mbfir.torchsim.abr2(rf, g, x, y, scales=(0.9, 1.0, 1.1))        # (S, nx, ny) each, abr2_batch's bits
    loss = ((2 * a.conj() * b - target).abs() ** 2).sum()
    loss.backward()                                                       # rf.grad and g.grad = dL/dgx + i dL/dgy
"""
import functools

import numpy as np


def _host(v, dtype):
    """A tensor, array or sequence as a host NumPy array (None stays None)."""
    if v is None:
        return None
    if hasattr(v, "detach"):
        import torch
        if torch._C._functorch.is_functorch_wrapped_tensor(v):           # torch.func's transforms wrap what jvp receives: the
            from torch._functorch.pyfunctorch import retrieve_current_functorch_interpreter          # values lie one level down
            with retrieve_current_functorch_interpreter().lower():
                return _host(torch._C._functorch.get_unwrapped(v), dtype)
        v = v.detach().resolve_conj().resolve_neg().cpu().numpy()       # autograd hands lazily conjugated cotangents on
    return np.asarray(v, dtype=dtype)


def _has_tangent(v):
    """Whether the tensor v carries a forward-mode tangent (a torch.autograd.forward_ad dual tensor, or what torch.func.jvp hands on)"""
    import torch
    return torch.autograd.forward_ad.unpack_dual(v).tangent is not None


@functools.lru_cache(maxsize=None)
def _functions():
    """The two autograd.Function classes, built when torch is first needed.  forward and setup_context are separate, which
    torch.func's transforms require; backward and jvp read what setup_context kept."""
    import torch

    import mbfir

    def check(rf):
        if not torch.is_tensor(rf) or rf.dtype != torch.complex128 or rf.dim() != 1:
            raise ValueError("torchsim: rf must be a 1-D complex128 tensor")

    def check_g(g, dtype, name):
        """g may be None, an array (a constant) or a tensor; one that requires grad must have the dtype its gradient comes in"""
        if torch.is_tensor(g) and g.requires_grad and (g.dtype != dtype or g.dim() != 1):
            raise ValueError("torchsim: a g that requires grad must be a 1-D %s tensor" % name)

    def tensors(rf, arrays):
        return tuple(torch.from_numpy(np.ascontiguousarray(v)).to(rf.device) for v in arrays)

    def no_g_tangent(vg):
        if vg is not None:
            raise NotImplementedError("torchsim: the forward-mode tangent with respect to g is not implemented (reverse mode is)")

    class Abr(torch.autograd.Function):
        @staticmethod
        def forward(rf, x, g, scales, hard_pulse):
            check(rf)
            check_g(g, torch.float64, "float64")
            x, g, scales, hard_pulse = _host(x, np.float64), _host(g, np.float64), tuple(scales), bool(hard_pulse)
            rfh = _host(rf, np.complex128)
            (a, b), = mbfir.abr_batch([rfh if g is None else (rfh, g)], x, scales=scales, hard_pulse=hard_pulse)
            return tensors(rf, (a, b))

        @staticmethod
        def setup_context(ctx, inputs, output):
            rf, x, g, scales, hard_pulse = inputs
            ctx.args = (_host(x, np.float64), _host(g, np.float64), tuple(scales), bool(hard_pulse))
            ctx.g_like = (g.shape, g.device) if torch.is_tensor(g) else None          # where g's gradient goes
            ctx.save_for_backward(rf)
            ctx.save_for_forward(rf)

        @staticmethod
        def jvp(ctx, v, vx, vg, *_):
            no_g_tangent(vg)
            rf, = ctx.saved_tensors
            x, g, scales, hard_pulse = ctx.args
            rfh = _host(rf, np.complex128)
            (_, tan), = mbfir.abr_jvp_batch([rfh if g is None else (rfh, g)], x, [_host(v, np.complex128)], scales=scales,
                                            hard_pulse=hard_pulse)
            return tensors(rf, tan)

        @staticmethod
        def backward(ctx, ca, cb):
            rf, = ctx.saved_tensors
            x, g, scales, hard_pulse = ctx.args
            rfh = _host(rf, np.complex128)
            pulses, cot = [rfh if g is None else (rfh, g)], [(_host(ca, np.complex128), _host(cb, np.complex128))]
            if not ctx.needs_input_grad[2]:
                grad, = mbfir.abr_vjp_batch(pulses, x, cot, scales=scales, hard_pulse=hard_pulse)
                return tensors(rf, (grad,)) + (None, None, None, None)
            (grad, gg), = mbfir.abr_vjp_rfg_batch(pulses, x, cot, scales=scales, hard_pulse=hard_pulse)
            grad, = tensors(rf, (grad,)) if ctx.needs_input_grad[0] else (None,)
            return grad, None, torch.from_numpy(gg.reshape(ctx.g_like[0])).to(ctx.g_like[1]), None, None

    class Abr2(torch.autograd.Function):
        @staticmethod
        def forward(rf, g, x, y, scales, hard_pulse):
            check(rf)
            check_g(g, torch.complex128, "complex128")
            g, x, y = _host(g, np.complex128), _host(x, np.float64), _host(y, np.float64)
            rfh = _host(rf, np.complex128)
            (a, b), = mbfir.abr2_batch([rfh if g is None else (rfh, g)], x, y, scales=tuple(scales), hard_pulse=bool(hard_pulse))
            return tensors(rf, (a, b))

        @staticmethod
        def setup_context(ctx, inputs, output):
            rf, g, x, y, scales, hard_pulse = inputs
            ctx.args = (_host(g, np.complex128), _host(x, np.float64), _host(y, np.float64), tuple(scales), bool(hard_pulse))
            ctx.g_like = (g.shape, g.device) if torch.is_tensor(g) else None          # where g's gradient goes
            ctx.save_for_backward(rf)
            ctx.save_for_forward(rf)

        @staticmethod
        def jvp(ctx, v, vg, *_):
            no_g_tangent(vg)
            rf, = ctx.saved_tensors
            g, x, y, scales, hard_pulse = ctx.args
            rfh = _host(rf, np.complex128)
            (_, tan), = mbfir.abr2_jvp_batch([rfh if g is None else (rfh, g)], x, y, [_host(v, np.complex128)], scales=scales,
                                             hard_pulse=hard_pulse)
            return tensors(rf, tan)

        @staticmethod
        def backward(ctx, ca, cb):
            rf, = ctx.saved_tensors
            g, x, y, scales, hard_pulse = ctx.args
            rfh = _host(rf, np.complex128)
            pulses, cot = [rfh if g is None else (rfh, g)], [(_host(ca, np.complex128), _host(cb, np.complex128))]
            if not ctx.needs_input_grad[1]:
                grad, = mbfir.abr2_vjp_batch(pulses, x, y, cot, scales=scales, hard_pulse=hard_pulse)
                return tensors(rf, (grad,)) + (None, None, None, None, None)
            (grad, gg), = mbfir.abr2_vjp_rfg_batch(pulses, x, y, cot, scales=scales, hard_pulse=hard_pulse)
            grad, = tensors(rf, (grad,)) if ctx.needs_input_grad[0] else (None,)
            return grad, torch.from_numpy(gg.reshape(ctx.g_like[0])).to(ctx.g_like[1]), None, None, None, None

    return Abr, Abr2


@functools.lru_cache(maxsize=None)
def _bloch_function():
    """The two autograd.Function classes of `bloch` (reverse mode only; with a forward-mode tangent), built when torch is first
    needed (forward and setup_context separate, as above)."""
    import torch

    import mbfir

    class Bloch(torch.autograd.Function):
        @staticmethod
        def forward(b1, m0, gr, df, rest, dp, scales):
            if not torch.is_tensor(b1) or b1.dtype != torch.complex128 or b1.dim() != 1:
                raise ValueError("torchsim: b1 must be a 1-D complex128 tensor")
            if torch.is_tensor(m0) and m0.requires_grad and (m0.dtype != torch.float64 or m0.dim() != 3 or m0.shape[0] != 3):
                raise ValueError("torchsim: an m0 that requires grad must be a float64 tensor of shape (3, nf, npos)")
            if torch.is_tensor(gr) and gr.requires_grad and (gr.dtype != torch.float64 or gr.dim() not in (1, 2) or
                                                             (gr.dim() == 2 and gr.shape[1] > 3)):
                raise ValueError("torchsim: a gr that requires grad must be a float64 tensor of shape (n,) or (n, 1..3)")
            if torch.is_tensor(df) and df.requires_grad and (df.dtype != torch.float64 or df.dim() != 1):
                raise ValueError("torchsim: a df that requires grad must be a float64 tensor of shape (nf,)")
            m0h = _host(m0, np.float64)
            res, = mbfir.bloch_batch([(_host(b1, np.complex128), _host(gr, np.float64)) + rest], _host(df, np.float64), dp,
                                     scales=scales, m0=None if m0h is None else tuple(m0h))
            return tuple(torch.from_numpy(np.ascontiguousarray(v)).to(b1.device) for v in res)

        @staticmethod
        def setup_context(ctx, inputs, output):
            b1, m0, gr, df, rest, dp, scales = inputs
            ctx.args = (_host(m0, np.float64), (_host(gr, np.float64),) + rest, _host(df, np.float64), dp, scales)
            ctx.m0_like = (m0.shape, m0.device) if torch.is_tensor(m0) else None          # where m0's gradient goes
            ctx.gr_like = (gr.shape, gr.device) if torch.is_tensor(gr) else None          # and gr's, and df's
            ctx.df_like = (df.shape, df.device) if torch.is_tensor(df) else None
            ctx.save_for_backward(b1)

        @staticmethod
        def jvp(ctx, *tangents):
            raise NotImplementedError("torchsim: the forward-mode tangent of bloch is not implemented (reverse mode is)")

        @staticmethod
        def backward(ctx, cx, cy, cz):
            b1, = ctx.saved_tensors
            m0h, pulse, df, dp, scales = ctx.args
            want_m0, want_gr, want_df = ctx.needs_input_grad[1:4]
            cot = tuple(_host(c, np.float64) for c in (cx, cy, cz))
            pulses, m0a = [(_host(b1, np.complex128),) + pulse], None if m0h is None else tuple(m0h)
            ggr = gdf = None
            if not (want_gr or want_df):                                # the b1 call, with its bits
                res, = mbfir.bloch_vjp_batch(pulses, df, dp, [cot], scales=scales, m0=m0a, grad_m0=want_m0)
                grad, gm = res if want_m0 else (res, None)
            else:                                                       # one call for every gradient that is wanted (section 8w)
                res, = mbfir.bloch_vjp_gr_batch(pulses, df, dp, [cot], scales=scales, m0=m0a, grad_m0=want_m0, grad_df=want_df)
                grad, gm = res[0], res[2] if want_m0 else None
                if want_gr:                                             # cut to the axes gr has
                    shape, dev = ctx.gr_like
                    k = shape[1] if len(shape) == 2 else 1
                    ggr = torch.from_numpy(np.ascontiguousarray(res[1][:, :k]).reshape(shape)).to(dev)
                if want_df:                                             # one df serves every scale and position: their sum
                    gdf = torch.from_numpy(np.ascontiguousarray(res[-1].sum(axis=(0, 2))).reshape(ctx.df_like[0])).to(ctx.df_like[1])
            gb = torch.from_numpy(np.ascontiguousarray(grad)).to(b1.device) if ctx.needs_input_grad[0] else None
            if want_m0:                                                 # one m0 serves every scale: its gradient is their sum
                gm = torch.from_numpy(np.stack([v.sum(0) for v in gm]).reshape(ctx.m0_like[0])).to(ctx.m0_like[1])
            return gb, gm, ggr, gdf, None, None, None

    class BlochForward(Bloch):
        """Bloch with a forward-mode tangent: the same forward and backward, plus a jvp that is one mbfir.bloch_jvp_batch call with
        one direction, in b1 and, when m0 is a tensor with a tangent, in m0."""

        @staticmethod
        def setup_context(ctx, inputs, output):
            Bloch.setup_context(ctx, inputs, output)
            ctx.save_for_forward(inputs[0])

        @staticmethod
        def jvp(ctx, v, vm0, vgr, vdf, *_):
            if vgr is not None or vdf is not None:
                raise NotImplementedError("torchsim: the forward-mode tangent with respect to gr or df is not implemented "
                                          "(reverse mode is)")
            b1, = ctx.saved_tensors
            m0h, pulse, df, dp, scales = ctx.args
            b1h = _host(b1, np.complex128)
            vh = np.zeros_like(b1h) if v is None else _host(v, np.complex128)
            dm0 = None if vm0 is None else [tuple(_host(vm0, np.float64))]
            (_, tan), = mbfir.bloch_jvp_batch([(b1h,) + pulse], df, dp, [vh], scales=scales,
                                              m0=None if m0h is None else tuple(m0h), tangents_m0=dm0)
            return tuple(torch.from_numpy(np.ascontiguousarray(t)).to(b1.device) for t in tan)

    class BlochSteady(torch.autograd.Function):
        """The steady state (bloch_batch mode 1): the backward is one mbfir.bloch_ss_vjp_batch call."""

        @staticmethod
        def forward(b1, pulse, df, dp, scales):
            if not torch.is_tensor(b1) or b1.dtype != torch.complex128 or b1.dim() != 1:
                raise ValueError("torchsim: b1 must be a 1-D complex128 tensor")
            res, = mbfir.bloch_batch([(_host(b1, np.complex128),) + pulse], df, dp, scales=scales, mode=1)
            return tuple(torch.from_numpy(np.ascontiguousarray(v)).to(b1.device) for v in res)

        @staticmethod
        def setup_context(ctx, inputs, output):
            b1, pulse, df, dp, scales = inputs
            ctx.args = (pulse, df, dp, scales)
            ctx.save_for_backward(b1)

        @staticmethod
        def jvp(ctx, *tangents):
            raise NotImplementedError("torchsim: the forward-mode tangent of bloch is not implemented (reverse mode is)")

        @staticmethod
        def backward(ctx, cx, cy, cz):
            b1, = ctx.saved_tensors
            pulse, df, dp, scales = ctx.args
            cot = tuple(_host(c, np.float64) for c in (cx, cy, cz))
            grad, = mbfir.bloch_ss_vjp_batch([(_host(b1, np.complex128),) + pulse], df, dp, [cot], scales=scales)
            return torch.from_numpy(np.ascontiguousarray(grad)).to(b1.device), None, None, None, None

    class BlochSteadyForward(BlochSteady):
        """BlochSteady with a forward-mode tangent: a jvp that is one mbfir.bloch_ss_jvp_batch call with one direction."""

        @staticmethod
        def setup_context(ctx, inputs, output):
            BlochSteady.setup_context(ctx, inputs, output)
            ctx.save_for_forward(inputs[0])

        @staticmethod
        def jvp(ctx, v, *_):
            b1, = ctx.saved_tensors
            pulse, df, dp, scales = ctx.args
            b1h = _host(b1, np.complex128)
            vh = np.zeros_like(b1h) if v is None else _host(v, np.complex128)
            (_, tan), = mbfir.bloch_ss_jvp_batch([(b1h,) + pulse], df, dp, [vh], scales=scales)
            return tuple(torch.from_numpy(np.ascontiguousarray(t)).to(b1.device) for t in tan)

    class BlochSteadyG(torch.autograd.Function):
        """The steady state with gr and / or df as inputs of the graph: the forward is BlochSteady's, the backward one
        mbfir.bloch_ss_vjp_gr_batch call for every gradient that is wanted."""

        @staticmethod
        def forward(b1, gr, df, rest, dp, scales):
            if not torch.is_tensor(b1) or b1.dtype != torch.complex128 or b1.dim() != 1:
                raise ValueError("torchsim: b1 must be a 1-D complex128 tensor")
            if torch.is_tensor(gr) and gr.requires_grad and (gr.dtype != torch.float64 or gr.dim() not in (1, 2) or
                                                             (gr.dim() == 2 and gr.shape[1] > 3)):
                raise ValueError("torchsim: a gr that requires grad must be a float64 tensor of shape (n,) or (n, 1..3)")
            if torch.is_tensor(df) and df.requires_grad and (df.dtype != torch.float64 or df.dim() != 1):
                raise ValueError("torchsim: a df that requires grad must be a float64 tensor of shape (nf,)")
            res, = mbfir.bloch_batch([(_host(b1, np.complex128), _host(gr, np.float64)) + rest], _host(df, np.float64), dp,
                                     scales=scales, mode=1)
            return tuple(torch.from_numpy(np.ascontiguousarray(v)).to(b1.device) for v in res)

        @staticmethod
        def setup_context(ctx, inputs, output):
            b1, gr, df, rest, dp, scales = inputs
            ctx.args = ((_host(gr, np.float64),) + rest, _host(df, np.float64), dp, scales)
            ctx.gr_like = (gr.shape, gr.device) if torch.is_tensor(gr) else None          # where gr's gradient goes, and df's
            ctx.df_like = (df.shape, df.device) if torch.is_tensor(df) else None
            ctx.out_shape = tuple(output[0].shape)                       # of a cotangent that arrives as None (BlochSteadyGForward)
            ctx.save_for_backward(b1)

        @staticmethod
        def jvp(ctx, *tangents):
            raise NotImplementedError("torchsim: the forward-mode tangent of bloch is not implemented (reverse mode is)")

        @staticmethod
        def backward(ctx, cx, cy, cz):
            b1, = ctx.saved_tensors
            pulse, df, dp, scales = ctx.args
            want_gr, want_df = ctx.needs_input_grad[1:3]
            cot = tuple(np.zeros(ctx.out_shape) if c is None else _host(c, np.float64) for c in (cx, cy, cz))
            pulses = [(_host(b1, np.complex128),) + pulse]
            ggr = gdf = None
            if not (want_gr or want_df):                                # the b1 call, with its bits
                grad, = mbfir.bloch_ss_vjp_batch(pulses, df, dp, [cot], scales=scales)
            else:
                res, = mbfir.bloch_ss_vjp_gr_batch(pulses, df, dp, [cot], scales=scales, grad_df=want_df)
                grad = res[0]
                if want_gr:                                             # cut to the axes gr has
                    shape, dev = ctx.gr_like
                    k = shape[1] if len(shape) == 2 else 1
                    ggr = torch.from_numpy(np.ascontiguousarray(res[1][:, :k]).reshape(shape)).to(dev)
                if want_df:                                             # one df serves every scale and position: their sum
                    gdf = torch.from_numpy(np.ascontiguousarray(res[2].sum(axis=(0, 2))).reshape(ctx.df_like[0])).to(ctx.df_like[1])
            gb = torch.from_numpy(np.ascontiguousarray(grad)).to(b1.device) if ctx.needs_input_grad[0] else None
            return gb, ggr, gdf, None, None, None

    class BlochSteadyGForward(BlochSteadyG):
        """BlochSteadyG with the forward-mode tangent in b1, one mbfir.bloch_ss_jvp_batch call with one direction; a tangent for gr
        or df raises NotImplementedError."""

        @staticmethod
        def setup_context(ctx, inputs, output):
            BlochSteadyG.setup_context(ctx, inputs, output)
            ctx.save_for_forward(inputs[0])
            ctx.set_materialize_grads(False)                            # a gr or df without a tangent arrives as None, not as zeros

        @staticmethod
        def jvp(ctx, v, vgr, vdf, *_):
            if vgr is not None or vdf is not None:
                raise NotImplementedError("torchsim: the forward-mode tangent with respect to gr or df is not implemented "
                                          "(reverse mode is)")
            b1, = ctx.saved_tensors
            pulse, df, dp, scales = ctx.args
            b1h = _host(b1, np.complex128)
            vh = np.zeros_like(b1h) if v is None else _host(v, np.complex128)
            (_, tan), = mbfir.bloch_ss_jvp_batch([(b1h,) + pulse], df, dp, [vh], scales=scales)
            return tuple(torch.from_numpy(np.ascontiguousarray(t)).to(b1.device) for t in tan)

    return Bloch, BlochForward, BlochSteady, BlochSteadyForward, BlochSteadyG, BlochSteadyGForward


def bloch(b1, gr, tp, t1, t2, df, dp, *, nucleus="C-13", scales=(1.0,), m0=None, forward_mode=False, steady_state=False):
    """(mx, my, mz) of mbfir.bloch_batch([(b1, gr, tp, t1, t2, nucleus)], df, dp, scales=scales, m0=m0), the end point of the Bloch
    simulation with relaxation, each a float64 tensor of shape (S, nf, npos) with bloch_batch's bits.  Differentiable in reverse mode
    in b1 (a 1-D complex128 tensor) and in m0 when that is a float64 tensor of shape (3, nf, npos) that requires grad (its gradient
    is summed over the scales); the backward is one mbfir.bloch_vjp_batch call.  Any other m0 ((mx, my, mz) or
    an array of shape (3, nf, npos); None: equilibrium), tp, t1, t2 and dp are constants.  gr and df are constants too unless they
    are float64 tensors that require grad, gr of shape (n,) or (n, 1..3) and df of shape (nf,) (another dtype or shape raises
    ValueError): then they are differentiated in reverse mode as well, gr's gradient cut to its shape and df's summed over the
    scales and positions, and the backward is one mbfir.bloch_vjp_gr_batch call (section 8w); a forward-mode tangent for either
    raises NotImplementedError.  A forward-mode tangent raises
    NotImplementedError unless forward_mode is set: then torch.func.jvp and torch.autograd.forward_ad dual tensors pass through as
    well, the tangent in b1 and in a tensor m0 being one mbfir.bloch_jvp_batch call with one direction (section 8q).
    With steady_state the result is the steady state of the period b1 instead, bloch_batch(mode=1) with its bits (for balanced SSFP
    the period is the pulse plus the dead time of one repetition): differentiable in b1, the backward being one
    mbfir.bloch_ss_vjp_batch call and, with forward_mode, the tangent one mbfir.bloch_ss_jvp_batch call (section 8t).  A gr or df
    that is a float64 tensor requiring grad (shapes and ValueErrors as above) is differentiated in reverse mode there too, gr's
    gradient cut to its shape and df's summed over the scales and positions: the backward is then one mbfir.bloch_ss_vjp_gr_batch
    call for every gradient that is wanted (section 8x), and a forward-mode tangent for gr or df raises NotImplementedError; when
    neither requires grad the calls are the b1 ones, with their bits.  The steady state does not depend on m0: an m0 other than
    None raises ValueError."""
    if steady_state:
        if m0 is not None:
            raise ValueError("torchsim: the steady state does not depend on m0; pass m0=None with steady_state")
        if any(hasattr(v, "detach") and (v.requires_grad or _has_tangent(v)) for v in (gr, df)):      # inputs of the graph (section 8x)
            fn = _bloch_function()[5 if forward_mode else 4]
            gr = gr if hasattr(gr, "detach") else _host(gr, np.float64)
            df = df if hasattr(df, "detach") else _host(df, np.float64)
            return fn.apply(b1, gr, df, (_host(tp, np.float64), float(t1), float(t2), nucleus), _host(dp, np.float64), tuple(scales))
        pulse = (_host(gr, np.float64), _host(tp, np.float64), float(t1), float(t2), nucleus)
        fn = _bloch_function()[3 if forward_mode else 2]
        return fn.apply(b1, pulse, _host(df, np.float64), _host(dp, np.float64), tuple(scales))
    if m0 is not None and not hasattr(m0, "detach"):
        m0 = np.stack([np.asarray(v, dtype=np.float64) for v in m0])
    fn = _bloch_function()[1 if forward_mode else 0]
    gr = gr if hasattr(gr, "detach") else _host(gr, np.float64)       # a tensor stays an input of the graph
    df = df if hasattr(df, "detach") else _host(df, np.float64)
    return fn.apply(b1, m0, gr, df, (_host(tp, np.float64), float(t1), float(t2), nucleus), _host(dp, np.float64), tuple(scales))


@functools.lru_cache(maxsize=None)
def _train_function():
    """The autograd.Function class of `bloch_train`, built when torch is first needed (forward and setup_context separate, as
    above).  kw: the constants of the train as a tuple of (name, value) pairs."""
    import torch

    import mbfir

    class BlochTrain(torch.autograd.Function):
        @staticmethod
        def forward(b1, m0, rest, df, dp, ntr, kw, final):
            if not torch.is_tensor(b1) or b1.dtype != torch.complex128 or b1.dim() != 1:
                raise ValueError("torchsim: b1 must be a 1-D complex128 tensor")
            if torch.is_tensor(m0) and m0.requires_grad and (m0.dtype != torch.float64 or m0.dim() != 3 or m0.shape[0] != 3):
                raise ValueError("torchsim: an m0 that requires grad must be a float64 tensor of shape (3, nf, npos)")
            m0h = _host(m0, np.float64)
            res, = mbfir.bloch_train_batch([(_host(b1, np.complex128),) + rest], df, dp, ntr, m0=None if m0h is None else tuple(m0h),
                                           final=final, **dict(kw))
            planes = res[0] + res[1] if final else res
            return tuple(torch.from_numpy(np.ascontiguousarray(v)).to(b1.device) for v in planes)

        @staticmethod
        def setup_context(ctx, inputs, output):
            b1, m0, rest, df, dp, ntr, kw, final = inputs
            ctx.args = (_host(m0, np.float64), rest, df, dp, ntr, kw, final)
            ctx.m0_like = (m0.shape, m0.device) if torch.is_tensor(m0) else None          # where m0's gradient goes
            ctx.save_for_backward(b1)

        @staticmethod
        def jvp(ctx, *tangents):
            raise NotImplementedError("torchsim: the forward-mode tangent of bloch_train is not implemented (reverse mode is)")

        @staticmethod
        def backward(ctx, *cots):
            b1, = ctx.saved_tensors
            m0h, rest, df, dp, ntr, kw, final = ctx.args
            want_m0 = ctx.needs_input_grad[1]
            cot = tuple(_host(c, np.float64) for c in cots)
            res, = mbfir.bloch_train_vjp_batch([(_host(b1, np.complex128),) + rest], df, dp, ntr, [cot[:3]],
                                               cot_final=[cot[3:]] if final else None, m0=None if m0h is None else tuple(m0h),
                                               grad_m0=want_m0, **dict(kw))
            grad, gm = res if want_m0 else (res, None)
            gb = torch.from_numpy(np.ascontiguousarray(grad)).to(b1.device) if ctx.needs_input_grad[0] else None
            if want_m0:                                                 # one m0 serves every scale: its gradient is their sum
                gm = torch.from_numpy(np.stack([v.sum(0) for v in gm]).reshape(ctx.m0_like[0])).to(ctx.m0_like[1])
            return gb, gm, None, None, None, None, None, None

    return BlochTrain


@functools.lru_cache(maxsize=None)
def _train_forward_function():
    """BlochTrain with a forward-mode tangent: the same forward and backward, plus a jvp that is one mbfir.bloch_train_jvp_batch
    call with one direction, in b1 and, when m0 is a tensor with a tangent, in m0."""
    import torch

    import mbfir

    class BlochTrainForward(_train_function()):
        @staticmethod
        def setup_context(ctx, inputs, output):
            _train_function().setup_context(ctx, inputs, output)
            ctx.save_for_forward(inputs[0])

        @staticmethod
        def jvp(ctx, v, vm0, *_):
            b1, = ctx.saved_tensors
            m0h, rest, df, dp, ntr, kw, final = ctx.args
            b1h = _host(b1, np.complex128)
            vh = np.zeros_like(b1h) if v is None else _host(v, np.complex128)
            dm0 = None if vm0 is None else [tuple(_host(vm0, np.float64))]
            tan, = mbfir.bloch_train_jvp_batch([(b1h,) + rest], df, dp, ntr, [vh], tangents_m0=dm0,
                                               m0=None if m0h is None else tuple(m0h), final=final, **dict(kw))
            planes = tan[0] + tan[1] if final else tan
            return tuple(torch.from_numpy(np.ascontiguousarray(t)).to(b1.device) for t in planes)

    return BlochTrainForward


def _in_graph(v):
    """Whether v is a tensor that autograd follows: one that requires grad, a forward-mode dual or a torch.func-wrapped tensor"""
    if not hasattr(v, "detach"):
        return False
    import torch
    return bool(v.requires_grad or torch._C._functorch.is_functorch_wrapped_tensor(v)
                or torch.autograd.forward_ad.unpack_dual(v).tangent is not None)


@functools.lru_cache(maxsize=None)
def _train_sched_function():
    """BlochTrain with the schedule in the graph: gains and phases (each a float64 tensor of shape (ntr,), or a constant) are inputs.
    The backward is one mbfir.bloch_train_vjp_sched_batch call when either needs a gradient and the shipped
    mbfir.bloch_train_vjp_batch call when b1 or m0 does.  kw: the train's other constants."""
    import torch

    import mbfir

    def table(v, ntr, what):
        if torch.is_tensor(v) and v.requires_grad and (v.dtype != torch.float64 or v.shape != (ntr,)):
            raise ValueError("torchsim: %s that require grad must be a float64 tensor of shape (ntr,)" % what)
        return _host(v, np.float64)

    class BlochTrainSched(torch.autograd.Function):
        @staticmethod
        def forward(b1, m0, gains, phases, rest, df, dp, ntr, kw, final):
            gh, ph = table(gains, ntr, "gains"), table(phases, ntr, "phases")
            return _train_function().forward(b1, m0, rest, df, dp, ntr, kw + (("gains", gh), ("phases", ph)), final)

        @staticmethod
        def setup_context(ctx, inputs, output):
            b1, m0, gains, phases, rest, df, dp, ntr, kw, final = inputs
            kw = kw + (("gains", _host(gains, np.float64)), ("phases", _host(phases, np.float64)))
            ctx.args = (_host(m0, np.float64), rest, df, dp, ntr, kw, final)
            ctx.m0_like = (m0.shape, m0.device) if torch.is_tensor(m0) else None
            ctx.sched_like = tuple(v.device if torch.is_tensor(v) else None for v in (gains, phases))
            ctx.save_for_backward(b1)

        @staticmethod
        def jvp(ctx, *tangents):
            raise NotImplementedError("torchsim: the forward-mode tangent of bloch_train in the gains and the phases is not "
                                      "implemented (reverse mode is)")

        @staticmethod
        def backward(ctx, *cots):
            b1, = ctx.saved_tensors
            m0h, rest, df, dp, ntr, kw, final = ctx.args
            want_b1, want_m0, want_g, want_p = ctx.needs_input_grad[:4]
            cot = tuple(_host(c, np.float64) for c in cots)
            args = ([(_host(b1, np.complex128),) + rest], df, dp, ntr, [cot[:3]])
            kws = dict(kw, cot_final=[cot[3:]] if final else None, m0=None if m0h is None else tuple(m0h))
            gb = gm = gg = gp = None
            if want_g or want_p:
                res, = mbfir.bloch_train_vjp_sched_batch(*args, grad_gains=want_g, grad_phases=want_p, **kws)
                if want_g:
                    gg = torch.from_numpy(np.ascontiguousarray(res[0])).to(ctx.sched_like[0])
                if want_p:
                    gp = torch.from_numpy(np.ascontiguousarray(res[1])).to(ctx.sched_like[1])
            if want_b1 or want_m0:
                res, = mbfir.bloch_train_vjp_batch(*args, grad_m0=want_m0, **kws)
                grad, gm = res if want_m0 else (res, None)
                gb = torch.from_numpy(np.ascontiguousarray(grad)).to(b1.device) if want_b1 else None
                if want_m0:                                             # one m0 serves every scale: its gradient is their sum
                    gm = torch.from_numpy(np.stack([v.sum(0) for v in gm]).reshape(ctx.m0_like[0])).to(ctx.m0_like[1])
            return gb, gm, gg, gp, None, None, None, None, None, None

    return BlochTrainSched


@functools.lru_cache(maxsize=None)
def _train_sched_forward_function():
    """BlochTrainSched with a forward-mode tangent: the same forward and backward, plus a jvp that is one
    mbfir.bloch_train_jvp_sched_batch call with one direction for the tangents of the gains, the phases and m0
    and, when b1 has a tangent too, one mbfir.bloch_train_jvp_batch call; the tangent is linear, so the two results are summed, m0's
    tangent going to one of the calls only.  Each call is asked only for what has a tangent."""
    import torch

    import mbfir

    base = _train_sched_function()

    class BlochTrainSchedForward(base):
        @staticmethod
        def setup_context(ctx, inputs, output):
            base.setup_context(ctx, inputs, output)
            ctx.save_for_forward(inputs[0])
            ctx.out_like = tuple((o.shape, o.device) for o in output)
            ctx.set_materialize_grads(False)                            # an input without a tangent arrives as None, not as zeros

        @staticmethod
        def backward(ctx, *cots):                                       # the parent's, on the zeros it would have been handed
            cots = tuple(torch.zeros(s, dtype=torch.float64, device=d) if c is None else c for c, (s, d) in zip(cots, ctx.out_like))
            return base.backward(ctx, *cots)

        @staticmethod
        def jvp(ctx, v, vm0, vg, vp, *_):
            b1, = ctx.saved_tensors
            m0h, rest, df, dp, ntr, kw, final = ctx.args
            pulses = [(_host(b1, np.complex128),) + rest]
            kws = dict(kw, m0=None if m0h is None else tuple(m0h), final=final)
            dm0 = None if vm0 is None else [tuple(_host(vm0, np.float64))]
            sched = vg is not None or vp is not None or (dm0 is not None and v is None)
            planes = None
            if sched:
                tan, = mbfir.bloch_train_jvp_sched_batch(pulses, df, dp, ntr,
                                                         tangents_gains=None if vg is None else [_host(vg, np.float64)],
                                                         tangents_phases=None if vp is None else [_host(vp, np.float64)],
                                                         tangents_m0=dm0, **kws)
                planes = tan[0] + tan[1] if final else tan
            if v is not None:
                tan, = mbfir.bloch_train_jvp_batch(pulses, df, dp, ntr, [_host(v, np.complex128)], tangents_m0=None if sched else dm0,
                                                   **kws)
                more = tan[0] + tan[1] if final else tan
                planes = more if planes is None else tuple(a + b for a, b in zip(planes, more))
            return tuple(torch.from_numpy(np.ascontiguousarray(t)).to(b1.device) for t in planes)

    return BlochTrainSchedForward


@functools.lru_cache(maxsize=None)
def _train_g_function():
    """BlochTrain with gr and / or df as inputs of the graph: the forward is BlochTrain's, the backward one
    mbfir.bloch_train_vjp_gr_batch call for every gradient that is wanted, or the shipped
    mbfir.bloch_train_vjp_batch call when neither gr nor df needs one.  rest: (tp, t1, t2, nucleus)."""
    import torch

    import mbfir

    class BlochTrainG(torch.autograd.Function):
        @staticmethod
        def forward(b1, m0, gr, df, rest, dp, ntr, kw, final):
            if torch.is_tensor(gr) and gr.requires_grad and (gr.dtype != torch.float64 or gr.dim() not in (1, 2) or
                                                             (gr.dim() == 2 and gr.shape[1] > 3)):
                raise ValueError("torchsim: a gr that requires grad must be a float64 tensor of shape (n,) or (n, 1..3)")
            if torch.is_tensor(df) and df.requires_grad and (df.dtype != torch.float64 or df.dim() != 1):
                raise ValueError("torchsim: a df that requires grad must be a float64 tensor of shape (nf,)")
            return _train_function().forward(b1, m0, (_host(gr, np.float64),) + rest, _host(df, np.float64), dp, ntr, kw, final)

        @staticmethod
        def setup_context(ctx, inputs, output):
            b1, m0, gr, df, rest, dp, ntr, kw, final = inputs
            ctx.args = (_host(m0, np.float64), (_host(gr, np.float64),) + rest, _host(df, np.float64), dp, ntr, kw, final)
            ctx.m0_like = (m0.shape, m0.device) if torch.is_tensor(m0) else None          # where the gradients go
            ctx.gr_like = (gr.shape, gr.device) if torch.is_tensor(gr) else None
            ctx.df_like = (df.shape, df.device) if torch.is_tensor(df) else None
            ctx.save_for_backward(b1)

        @staticmethod
        def jvp(ctx, *tangents):
            raise NotImplementedError("torchsim: the forward-mode tangent of bloch_train with respect to gr or df is not implemented "
                                      "(reverse mode is)")

        @staticmethod
        def backward(ctx, *cots):
            b1, = ctx.saved_tensors
            m0h, rest, df, dp, ntr, kw, final = ctx.args
            want_b1, want_m0, want_gr, want_df = ctx.needs_input_grad[:4]
            cot = tuple(_host(c, np.float64) for c in cots)
            args = ([(_host(b1, np.complex128),) + rest], df, dp, ntr, [cot[:3]])
            kws = dict(kw, cot_final=[cot[3:]] if final else None, m0=None if m0h is None else tuple(m0h), grad_m0=want_m0)
            gm = ggr = gdf = None
            if not (want_gr or want_df):                                # the b1 call, with its bits
                res, = mbfir.bloch_train_vjp_batch(*args, **kws)
                grad, gm = res if want_m0 else (res, None)
            else:
                res, = mbfir.bloch_train_vjp_gr_batch(*args, grad_df=want_df, **kws)
                grad = res[0]
                gm = res[2] if want_m0 else None
                if want_gr:                                             # cut to the axes gr has
                    shape, dev = ctx.gr_like
                    k = shape[1] if len(shape) == 2 else 1
                    ggr = torch.from_numpy(np.ascontiguousarray(res[1][:, :k]).reshape(shape)).to(dev)
                if want_df:                                             # one df serves every scale and position: their sum
                    gdf = torch.from_numpy(np.ascontiguousarray(res[-1].sum(axis=(0, 2))).reshape(ctx.df_like[0])).to(ctx.df_like[1])
            gb = torch.from_numpy(np.ascontiguousarray(grad)).to(b1.device) if want_b1 else None
            if want_m0:                                                 # one m0 serves every scale: its gradient is their sum
                gm = torch.from_numpy(np.stack([v.sum(0) for v in gm]).reshape(ctx.m0_like[0])).to(ctx.m0_like[1])
            return gb, gm, ggr, gdf, None, None, None, None, None

    return BlochTrainG


@functools.lru_cache(maxsize=None)
def _train_g_forward_function():
    """BlochTrainG with the forward-mode tangent in b1 and in a tensor m0, one mbfir.bloch_train_jvp_batch call with one direction
    (DESIGN section 8aa); a tangent for gr or df raises NotImplementedError."""
    import torch

    import mbfir

    base = _train_g_function()

    class BlochTrainGForward(base):
        @staticmethod
        def setup_context(ctx, inputs, output):
            base.setup_context(ctx, inputs, output)
            ctx.save_for_forward(inputs[0])
            ctx.out_like = tuple((o.shape, o.device) for o in output)
            ctx.set_materialize_grads(False)                            # a gr or df without a tangent arrives as None, not as zeros

        @staticmethod
        def backward(ctx, *cots):                                       # the parent's, on the zeros it would have been handed
            cots = tuple(torch.zeros(s, dtype=torch.float64, device=d) if c is None else c for c, (s, d) in zip(cots, ctx.out_like))
            return base.backward(ctx, *cots)

        @staticmethod
        def jvp(ctx, v, vm0, vgr, vdf, *_):
            if vgr is not None or vdf is not None:
                raise NotImplementedError("torchsim: the forward-mode tangent of bloch_train with respect to gr or df is not "
                                          "implemented (reverse mode is)")
            b1, = ctx.saved_tensors
            m0h, rest, df, dp, ntr, kw, final = ctx.args
            b1h = _host(b1, np.complex128)
            vh = np.zeros_like(b1h) if v is None else _host(v, np.complex128)
            dm0 = None if vm0 is None else [tuple(_host(vm0, np.float64))]
            tan, = mbfir.bloch_train_jvp_batch([(b1h,) + rest], df, dp, ntr, [vh], tangents_m0=dm0,
                                               m0=None if m0h is None else tuple(m0h), final=final, **dict(kw))
            planes = tan[0] + tan[1] if final else tan
            return tuple(torch.from_numpy(np.ascontiguousarray(t)).to(b1.device) for t in planes)

    return BlochTrainGForward


def bloch_train(b1, gr, tp, t1, t2, df, dp, ntr, *, nucleus="C-13", phases=np.pi, gains=1.0, echo=None, scales=(1.0,), m0=None,
                meq=1.0, demod=False, final=False, forward_mode=False):
    """The echoes (mx, my, mz) of mbfir.bloch_train_batch([(b1, gr, tp, t1, t2, nucleus)], df, dp, ntr, ...), each a float64 tensor
    of shape (S, ntr, nf, npos) with bloch_train_batch's bits; with final, ((mx, my, mz), (fx, fy, fz)), the second being the state
    after the last repetition, each of shape (S, nf, npos).  Differentiable in reverse mode in b1 (a 1-D complex128 tensor) and in
    m0 when that is a float64 tensor of shape (3, nf, npos) that requires grad (its gradient is summed over the scales); the
    backward is one mbfir.bloch_train_vjp_batch call.  Every other argument is a constant of the graph: gr, tp,
    t1, t2, df, dp, ntr, the phases, the gains, echo, the scales, meq, and an m0 given as (mx, my, mz), as an array of shape (3, nf,
    npos) or as None (equilibrium).  A forward-mode tangent raises NotImplementedError unless forward_mode is set: then
    torch.func.jvp and torch.autograd.forward_ad dual tensors pass through as well, the tangent in b1 and in a tensor m0 being one
    mbfir.bloch_train_jvp_batch call with one direction (section 8aa).  gains and phases may also be float64 tensors of shape
    (ntr,) that require grad: the schedule is then differentiated in reverse mode, per repetition, by one
    mbfir.bloch_train_vjp_sched_batch call (section 8ad), next to the call for b1 and m0 when those need gradients too.  A
    forward-mode tangent in the schedule raises NotImplementedError unless forward_mode is set: then the tangent in the gains, the
    phases and m0 is one mbfir.bloch_train_jvp_sched_batch call with one direction (section 8ae), summed with one
    mbfir.bloch_train_jvp_batch call when b1 has a tangent too; reverse mode keeps its calls and its bits.
    gr and df may be float64 tensors that require grad, gr of shape (n,) or (n, 1..3) and df of shape (nf,) (another dtype or shape
    raises ValueError): then they are differentiated in reverse mode as well, gr's gradient cut to its shape and df's summed over
    the scales and positions, and the backward is one mbfir.bloch_train_vjp_gr_batch call for every gradient that is wanted
    (section 8aj); a backward that needs neither makes the b1 call.  A forward-mode tangent for gr or df raises
    NotImplementedError, with and without forward_mode, and so does a gr or df in the graph together with gains or phases in the
    graph: no call differentiates both."""
    if m0 is not None and not hasattr(m0, "detach"):
        m0 = np.stack([np.asarray(v, dtype=np.float64) for v in m0])
    if any(_in_graph(v) for v in (gr, df)):                             # inputs of the graph (section 8aj)
        if any(_in_graph(v) for v in (gains, phases)):
            raise NotImplementedError("torchsim: bloch_train differentiates gr and df, or the gains and the phases, not both in one "
                                      "call: no gradient would be dropped silently, so detach one of the two groups")
        kw = (("phases", _host(phases, np.float64)), ("gains", _host(gains, np.float64)), ("echo", echo), ("scales", tuple(scales)),
              ("meq", float(meq)), ("demod", bool(demod)))
        gr = gr if hasattr(gr, "detach") else _host(gr, np.float64)
        df = df if hasattr(df, "detach") else _host(df, np.float64)
        fn = _train_g_forward_function() if forward_mode else _train_g_function()
        out = fn.apply(b1, m0, gr, df, (_host(tp, np.float64), float(t1), float(t2), nucleus), _host(dp, np.float64), int(ntr), kw,
                       bool(final))
        return (out[:3], out[3:]) if final else out
    if any(_in_graph(v) for v in (gains, phases)):
        kw = (("echo", echo), ("scales", tuple(scales)), ("meq", float(meq)), ("demod", bool(demod)))
        rest = (_host(gr, np.float64), _host(tp, np.float64), float(t1), float(t2), nucleus)
        fn = _train_sched_forward_function() if forward_mode else _train_sched_function()
        out = fn.apply(b1, m0, gains, phases, rest, _host(df, np.float64), _host(dp, np.float64), int(ntr), kw, bool(final))
        return (out[:3], out[3:]) if final else out
    kw =(("phases", _host(phases, np.float64)), ("gains", _host(gains, np.float64)), ("echo", echo), ("scales", tuple(scales)),
          ("meq", float(meq)), ("demod", bool(demod)))
    rest = (_host(gr, np.float64), _host(tp, np.float64), float(t1), float(t2), nucleus)
    fn = _train_forward_function() if forward_mode else _train_function()
    out = fn.apply(b1, m0, rest, _host(df, np.float64), _host(dp, np.float64), int(ntr), kw, bool(final))
    return (out[:3], out[3:]) if final else out


def abr(rf, x, g=None, *, scales=(1.0,), hard_pulse=False):
    """(a, b) of mbfir.abr_batch([rf or (rf, g)], x, scales=scales, hard_pulse=hard_pulse), each of shape (S, nx), as tensors that
    are differentiable in rf (a 1-D complex128 tensor) and, in reverse mode, in g (real, one weight per sample; None: 2 pi / n) when g
    is a 1-D float64 tensor that requires grad; any other g, and x, are constants."""
    return _functions()[0].apply(rf, x, g, scales, hard_pulse)


def abr2(rf, g, x, y, *, scales=(1.0,), hard_pulse=False):
    """(a, b) of mbfir.abr2_batch([rf or (rf, g)], x, y, scales=scales, hard_pulse=hard_pulse), each of shape (S, nx, ny), as
    tensors that are differentiable in rf (a 1-D complex128 tensor) and, in reverse mode, in g (complex: Re the x gradient, Im the
    y one; None: 2 pi / n along x) when g is a 1-D complex128 tensor that requires grad, its gradient being dL/dgx + i dL/dgy; any
    other g, x and y are constants."""
    return _functions()[1].apply(rf, g, x, y, scales, hard_pulse)
