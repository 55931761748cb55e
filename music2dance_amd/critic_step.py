"""The critic iteration as ONE hand-scheduled pass over the HIP kernels (no autograd tape).

The reference's critic iteration (phase3/train.py:204-216, phase2/train.py:146-155) is three critic
forwards (interpolated / real / fake poses) and three autograd passes (the penalty's first backward with
create_graph, its double backward, the loss backward), losses.py:28-44. The critics are piecewise linear
(conv / linear + ReLU, 'id' or 'relu' heads), so every one of those passes is the same linear operator chain
with fixed activation masks, and the whole iteration can be scheduled by hand:

  forward        pose branch ONCE over 3B rows [interpolated | real | fake] (m2d_pose_pack3 writes them
                 channels-first from the loader's (B, T, 69) poses and the generator's rows); audio branch
                 once over B rows (the audio is never interpolated: SURVEY.md A.6); head over 3B rows.
  backward-data  ONE chain for the pose branch: row cotangents 1 (interpolated rows: this IS the penalty's first
                 backward, d score / d input), -1/B (real), +1/B (fake: the loss backward). The skip
                 connections' gradients are added in the conv epilogues (m2d_conv1d_bwd_data_res).
  penalty        per-sample norms of the interpolated rows' input gradient (+ the audio term), loss scalars.
  tangent        the penalty's double backward is the forward-mode tangent G = d pen / d v pushed through the
                 linearised net: conv_fwd(G) with the forward's masks, written IN PLACE over the interpolated
                 rows of the saved activations (nothing reads those rows afterwards).
  weight grads   dW_n = correlate(x~_{n-1}, h_n) over all 3B rows in ONE launch per layer: rows [0, B) pair
                 (tangent, first-backward gradient) - the second-order term -, rows [B, 3B) pair (activation,
                 loss gradient) - the ordinary term. Bias gradients sum over the ordinary rows only
                 (m2d_conv1d_bwd_weight_from). No gradient-accumulation adds, no concatenations, no transposes.

Same arithmetic as the autograd path of losses.gradient_penalty + critic.score_pair (tests compare the two
gradient for gradient); ~100 launches per iteration instead of ~380.

Heads with `activ: tanh` (phase3/archis/default.py:309-310,339-340 of the reference) are not piecewise linear: with the
code e = tanh(u), the penalty's input gradient is v = A^T diag(1 - e^2) c (A the linearised branch up to u, c the
cotangent arriving from the fc1 / fc2 head), so its derivative has one more term than the tangent pairing above:
d pen = [tangent terms, the tangent passing through tanh as t_e = t_u (1 - e^2)] + <w, du>, w = t_u tanh''(u) c =
tanh_bwd(tanh_bwd_bwd(t_u, c, e), e) - an ORDINARY gradient of the interpolated rows with cotangent w at u. Those rows
then need both their tangent and their activations, so the pose branch runs on a 4B-row layout (activation side
[tangent | interpolated | real | fake], gradient side [first backward | tanh'' chain | real | fake]; row r pairs with
row r in the one weight-gradient launch per layer), the audio branch adds w to the cotangent of its forward half.

Structure. `CriticStep.run` is the SCHEDULE: row layout, what runs on the side stream and where it joins, the fc1 / fc2
head, loss scalars, tanh bookkeeping, where `on_grads` fires. The launch lists are in the two branch objects it calls
into, `PoseBranch` and `AudioBranch`: each resolves its layers' (weight, bias, stride, padding) once and holds one
pass's activation and gradient buffers between its sections. `_Grads` binds p.grad and calls `on_grads`.
`GanCriticStep` and `CondCriticStep` are schedules of their own over a `PoseBranch`.
"""
import contextlib

import torch

from . import kernels, levers, ops

ACT_NONE, ACT_RELU = ops.ACT_NONE, ops.ACT_RELU
K = kernels.impl


def _layer(conv):
    return conv.weight, conv.bias, conv.stride[0], conv.padding[0]


def _on(side):
    """the stream the enclosed launches (and allocations) go to: `side`, or the current one when there is none"""
    return torch.cuda.stream(side) if side is not None else contextlib.nullcontext()


def _cotangents(cache, B, dev, dtype, gamma, tanh=False):
    """-> (c1, cw, gamma): c1 (3B, 1) = the score cotangents of [interpolated | real | fake] = (1, -1/B, +1/B);
    cw = the same on the gradient-side row layout (tanh heads: (1, 0, -1/B, +1/B) over 4B rows, else c1)"""
    key = (B, str(dev), dtype)
    c = cache.get(key)
    if c is None:
        parts = [torch.ones(B), torch.full((B,), -1.0 / B), torch.full((B,), 1.0 / B)]
        c1 = torch.cat(parts).view(3 * B, 1).to(dev, dtype)
        cw = torch.cat([parts[0], torch.zeros(B)] + parts[1:]).view(4 * B, 1).to(dev, dtype) if tanh else c1
        c = cache[key] = (c1, cw, torch.tensor(gamma, dtype=dtype).to(dev))
    return c


class _Grads:
    """Binds p.grad as the weight-gradient launches are queued, in reverse parameter order, and tells `on_grads`
    (GradExchange.poll: buckets follow reverse parameter order too, so one can leave underneath the remaining launches).
    defer: gradients produced on the side stream are bound after the join (bind_late) - a bucket must not be packed on
    the main stream before the side stream's launches are ordered in front of it."""

    def __init__(self, on_grads):
        self.on_grads = on_grads
        self.late = []   # (parameter, gradient)

    def put(self, w, b, gw, gb, defer=False):
        if defer:
            self.late += ((w, gw), (b, gb))
        else:
            w.grad, b.grad = gw, gb

    def ready(self):
        if self.on_grads is not None:
            self.on_grads()

    def bind_late(self):
        for p, g in self.late:
            p.grad = g


class PoseBranch:
    """The launch lists of the pose branch: `stick` (a critic's stick_d, or a pose-only critic itself) = conv1, the
    residual blocks and the full-length conv (fconv / lastconv) behind them. One pass's buffers, each (R, CH, T): per
    block its input a[i], first conv's output p[i] and second conv's output q[i] (the activation masks), a[-1] the
    blocks' output; da[i] / dp[i] the gradients at a[i] / p[i] (da[0]: after conv1's ReLU); X the packed input rows."""

    def __init__(self, stick):
        self.conv1 = _layer(stick.conv1)
        self.blocks = [(_layer(blk.conv1), _layer(blk.conv2)) for blk in stick.blocks]
        fconv = stick.fconv if hasattr(stick, "fconv") else stick.lastconv
        self.fconv = (fconv.weight, fconv.bias)
        self.CH, self.C = self.conv1[0].shape[:2]
        self.Cc = fconv.weight.shape[0]
        self.release()

    def release(self):
        self.X = self.fw2d = self.a = self.p = self.q = self.da = self.dp = None

    def _rows(self):
        X = self.X
        return torch.empty((X.shape[0], self.CH, X.shape[2]), dtype=X.dtype, device=X.device)

    def forward(self, X, fw):
        """forward over rows `fw` of X (R, C, T) -> (a, p, q), written on rows `fw`"""
        k = K()
        self.X = X
        self.fw2d = self.fconv[0].view(self.Cc, self.CH * X.shape[2])
        w1, b1, _, pad1 = self.conv1
        a, p, q = [self._rows()], [], []
        k.conv1d_fwd(X[fw], w1, b1, 1, pad1, ACT_RELU, out=a[0][fw])
        for (wa, ba, _, pa), (wb, bb, _, pb) in self.blocks:
            pk, qk, ak = self._rows(), self._rows(), self._rows()
            k.conv1d_fwd(a[-1][fw], wa, ba, 1, pa, ACT_RELU, out=pk[fw])
            k.conv1d_fwd(pk[fw], wb, bb, 1, pb, ACT_RELU, residual=a[-1][fw], out=qk[fw], sum_out=ak[fw])
            p.append(pk)
            q.append(qk)
            a.append(ak)
        self.a, self.p, self.q = a, p, q
        return a, p, q

    def backward_data(self, c, rs=None, head=None):
        """backward-data chain for the (R, Cc) cotangents `c` at the full-length conv's output -> (da, dp).
        rs = None: all rows, into fresh gradient buffers; else rows `rs` only, of the existing ones (the tanh'' chain
        over the interpolated rows). head: what lies between the blocks and the full-length conv, applied to the
        gradient at the blocks' output (CondCriticStep: its dropout)"""
        k = K()
        a, p, q = self.a, self.p, self.q
        nb = len(self.blocks)
        T = a[0].shape[2]
        if rs is None:
            self.da = [self._rows() for _ in range(nb + 1)]
            self.dp = [self._rows() for _ in range(nb)]
        da, dp = self.da, self.dp
        sel = (lambda t: t) if rs is None else (lambda t: t[rs])
        k.gemm(1, sel(c), self.fw2d, out=sel(da[nb]).view(-1, self.CH * T))
        if head is not None:
            da[nb] = head(da[nb])
        for i in range(nb - 1, -1, -1):
            (wa, _, _, pa), (wb, _, _, pb) = self.blocks[i]
            k.conv1d_bwd_data(sel(da[i + 1]), wb, T, 1, pb, dy_mask=sel(q[i]), out_mask=sel(p[i]), out=sel(dp[i]))
            k.conv1d_bwd_data(sel(dp[i]), wa, T, 1, pa, residual=sel(da[i + 1]),
                              out_mask=sel(a[0]) if i == 0 else None, out=sel(da[i]))
        if nb == 0:   # (no conv epilogue to apply conv1's ReLU mask in)
            g = sel(da[0]) * (sel(a[0]) > 0)
            if rs is None:
                da[0] = g
            else:
                da[0][rs] = g
        return da, dp

    def input_grad(self, rs=None):
        """-> the gradient at the input rows (all, or rows `rs`): conv1's backward-data"""
        w1, _, _, pad1 = self.conv1
        return K().conv1d_bwd_data(self.da[0] if rs is None else self.da[0][rs], w1, self.X.shape[2], 1, pad1)

    def tangent(self, tg, mk):
        """the linearised branch applied to rows `tg` of X, with the activation masks of rows `mk`, written over rows
        `tg` of a / p (q keeps its masks)"""
        k = K()
        a, p, q = self.a, self.p, self.q
        w1, _, _, pad1 = self.conv1
        k.conv1d_fwd(self.X[tg], w1, None, 1, pad1, ACT_NONE, out_mask=a[0][mk], out=a[0][tg])
        for i, ((wa, _, _, pa), (wb, _, _, pb)) in enumerate(self.blocks):
            k.conv1d_fwd(a[i][tg], wa, None, 1, pa, ACT_NONE, out_mask=p[i][mk], out=p[i][tg])
            k.conv1d_fwd(p[i][tg], wb, None, 1, pb, ACT_NONE, residual=a[i][tg], out_mask=q[i][mk], out=a[i + 1][tg])

    def weight_grads(self, c, b0, grads, defer=False, head_in=None):
        """weight gradients, one launch per layer over all R rows, in reverse parameter order: c (R, Cc) the cotangents
        at the full-length conv's output. Bias gradients sum rows [b0, R) only (rows in front pair second-order
        operands). defer: bound after the join, and `on_grads` left to the caller (see _Grads); else it fires after each
        layer's. head_in: the full-length conv's input when it is not a[-1] (the dropped rows of CondCriticStep)"""
        k = K()
        a, p, q, da, dp = self.a, self.p, self.q, self.da, self.dp
        nb = len(self.blocks)
        R, CH, T = a[0].shape
        grads.put(*self.fconv, k.gemm(2, c, (a[nb] if head_in is None else head_in).view(R, CH * T)).view(self.fconv[0].shape),
                  k.channel_sums(c[b0:].contiguous()), defer=defer)
        if not defer:
            grads.ready()
        for i in range(nb - 1, -1, -1):
            (wa, ba, _, pa), (wb, bb, _, pb) = self.blocks[i]
            grads.put(wb, bb, *k.conv1d_bwd_weight(p[i], da[i + 1], wb.shape[2], 1, pb, dy_mask=q[i], with_bias=True,
                                                   bias_from_sample=b0), defer=defer)
            grads.put(wa, ba, *k.conv1d_bwd_weight(a[i], dp[i], wa.shape[2], 1, pa, with_bias=True,
                                                   bias_from_sample=b0), defer=defer)
            if not defer:
                grads.ready()
        w1, b1, _, pad1 = self.conv1
        grads.put(w1, b1, *k.conv1d_bwd_weight(self.X, da[0], w1.shape[2], 1, pad1, with_bias=True, bias_from_sample=b0),
                  defer=defer)


class AudioBranch:
    """The launch lists of the audio branch (audio_d: l1 .. l5 and the full-length l6). The audio is never interpolated,
    so the forward runs over B rows; every buffer has 2B rows all the same: Y[n] = [tangent | activation] of layer n,
    HD[n] = the gradients at Y[n], [first backward (the penalty's) | score backward], ca2 (2B, Ca) their cotangents at
    l6's output. Row r of Y pairs with row r of HD in the one weight-gradient launch per layer."""

    def __init__(self, au):
        self.layers = [_layer(conv) for conv in (au.l1, au.l2, au.l3, au.l4, au.l5)]
        self.l6 = (au.l6.weight, au.l6.bias)
        self.Ca = au.l6.weight.shape[0]
        self.release()

    def release(self):
        self.audio = self.w6 = self.Y = self.HD = self.ca2 = self.ga = self.lo = self.hi = None

    def flat(self, half):
        """rows `half` of the last conv's buffer as l6 sees them: (B, C5 * L5)"""
        return self.Y[4][half].view(self.B, -1)

    def forward(self, audio):
        k = K()
        B = self.B = audio.shape[0]
        self.audio = audio
        self.lo, self.hi = slice(0, B), slice(B, 2 * B)
        self.w6 = self.l6[0].view(self.Ca, -1)
        self.Y, x = [], audio
        for w, b, s_, pd in self.layers:
            Lo = kernels.conv_out_len(x.shape[2], w.shape[2], s_, pd)
            buf = torch.empty((2 * B, w.shape[0], Lo), dtype=audio.dtype, device=audio.device)
            x = k.conv1d_fwd(x, w, b, s_, pd, ACT_RELU, out=buf[B:])
            self.Y.append(buf)

    def seed(self, first, real, fake):
        """the cotangents at l6's output: `first` for the penalty's first backward, real + fake for the score backward
        (both poses were scored against the same audio)"""
        self.ca2 = torch.empty((2 * self.B, self.Ca), dtype=first.dtype, device=first.device)
        self.ca2[self.lo] = first
        torch.add(real, fake, out=self.ca2[self.hi])
        self.HD = [torch.empty_like(y) for y in self.Y]

    def chain(self, half):
        """backward-data down to l1's output for rows `half` of the gradient buffers; half = None: BOTH halves in one
        launch per layer - they pass through the same activation masks (the forward's, rows B: of Y), which the kernel
        reads once more for the second half (m2d_conv1d_bwd_data_shared_mask)"""
        k = K()
        B, Y, HD = self.B, self.Y, self.HD
        y5 = self.flat(self.hi)
        for hf in ((self.lo, self.hi) if half is None else (half,)):
            k.gemm(1, self.ca2[hf], self.w6, out_mask=y5, out=HD[4][hf].view(B, -1))
        sel = (lambda t: t) if half is None else (lambda t: t[half])
        for n in range(4, 0, -1):
            w, _, s_, pd = self.layers[n]
            k.conv1d_bwd_data(sel(HD[n]), w, Y[n - 1].shape[2], s_, pd, out_mask=Y[n - 1][B:], out=sel(HD[n - 1]))

    def input_grad(self):
        """-> the first backward's gradient at the audio: l1's backward-data"""
        w, _, s_, pd = self.layers[0]
        return K().conv1d_bwd_data(self.HD[0][self.lo], w, self.audio.shape[2], s_, pd)

    def tangent(self, ga):
        """the linearised convs applied to `ga` (the audio's shape), with the forward's masks, into rows [0, B) of Y"""
        k = K()
        B, Y = self.B, self.Y
        self.ga = x = ga
        for n, (w, _, s_, pd) in enumerate(self.layers):
            x = k.conv1d_fwd(x, w, None, s_, pd, ACT_NONE, out_mask=Y[n][B:], out=Y[n][0:B])

    def weight_grads(self, grads):
        """one launch per layer over the 2B rows, from l6 down; l1's two halves have different inputs (the tangent seed
        and the audio): two launches and an add"""
        k = K()
        B, Y, HD, ca2 = self.B, self.Y, self.HD, self.ca2
        grads.put(*self.l6, k.gemm(2, ca2, Y[4].view(2 * B, -1)).view(self.l6[0].shape),
                  k.channel_sums(ca2[B:].contiguous()))
        grads.ready()
        for n in range(4, 0, -1):
            w, b, s_, pd = self.layers[n]
            grads.put(w, b, *k.conv1d_bwd_weight(Y[n - 1], HD[n], w.shape[2], s_, pd, with_bias=True, bias_from_sample=B))
            grads.ready()
        w, b, s_, pd = self.layers[0]
        g2 = k.conv1d_bwd_weight(self.ga, HD[0][0:B], w.shape[2], s_, pd)
        g1, gb = k.conv1d_bwd_weight(self.audio, HD[0][B:], w.shape[2], s_, pd, with_bias=True)
        grads.put(w, b, g1.add_(g2), gb)


class CriticStep:
    """critic: phase3 SequenceDiscriminator / AblatedSequenceDiscriminator or phase2 SequenceDiscriminator."""

    @staticmethod
    def supports(critic):
        stick = getattr(critic, "stick_d", critic)
        if not hasattr(stick, "conv1") or not hasattr(stick, "blocks"):
            return False
        heads = [bool(getattr(b, "_head_tanh", False)) for b in (stick, getattr(critic, "audio_d", None)) if b is not None]
        if any(heads) and not (all(heads) and hasattr(critic, "fc1")):
            return False  # (both branches carry the same `activ`; a tanh head always feeds the fc1 / fc2 head)
        return True

    def __init__(self, critic, gamma, lp=False):
        assert self.supports(critic)
        self.critic = critic
        self.gamma = float(gamma)
        self.lp = bool(lp)
        stick = getattr(critic, "stick_d", critic)
        audio_d = getattr(critic, "audio_d", None)
        self.pose = PoseBranch(stick)
        self.audio = AudioBranch(audio_d) if audio_d is not None else None
        self.has_head = hasattr(critic, "fc1")
        self.head_act = int(getattr(stick, "_head_act", ACT_NONE))
        self.tanh = bool(getattr(stick, "_head_tanh", False))
        self._const = {}
        self.debug = None  # dev aid: a dict collects clones of the intermediates (tools/critic_step_debug.py)
        # the pose branch's launches are small (they leave most CUs idle between dependent kernels): they run on a
        # side stream underneath the audio branch's large convolutions, section by section
        self.overlap = self.audio is not None and getattr(type(critic), "overlap_branches", True)
        # the penalty's first backward and the score backward of the audio branch as ONE 2B-row launch per layer
        # (M2D_MERGE_AUDIO_BWD=0: two B-row chains, the round-4 schedule)
        self.merge_audio_chains = levers.on("M2D_MERGE_AUDIO_BWD")
        self._side = None
        self.join_pairs = None   # diagnostics (engine.timed_wait): how long the pose branch waited for the generator forward

    # ------------------------------------------------------------------ the two streams
    def _fork(self, dev):
        """-> (side stream or None, main stream); the side stream starts behind everything queued on main"""
        if not self.overlap or dev.type != "cuda":
            return None, None
        if self._side is None:
            # the critic's own pose-branch stream (its autograd path forks the same way): packed weight images are
            # cached per (weight, stream)
            if getattr(self.critic, "_stick_stream", None) is None:
                self.critic._stick_stream = torch.cuda.Stream(device=dev)
                self.critic._joins = {}
            self._side = self.critic._stick_stream
        cur = torch.cuda.current_stream(dev)
        self._side.wait_stream(cur)
        return self._side, cur

    @staticmethod
    def _join(side, cur, *tensors):
        if side is None:
            return
        cur.wait_stream(side)
        for t in tensors:
            if t is not None:
                t.record_stream(cur)

    def _wait_for(self, fake_ready, fake_rows, stream):
        """only the pose branch's stream waits for the generator forward"""
        if self.join_pairs is not None:
            from .engine import timed_wait
            timed_wait(stream, fake_ready, self.join_pairs)
        else:
            stream.wait_event(fake_ready)
        fake_rows.record_stream(stream)

    def _note(self, rows, **named):
        """dev aid: clones of rows `rows` of the named intermediates (a list as name0, name1, ...) into self.debug"""
        if self.debug is not None:
            for name, t in named.items():
                for i, x in enumerate(t if isinstance(t, list) else [] if t is None else [t]):
                    self.debug[name + (str(i) if isinstance(t, list) else "")] = x[rows].clone()

    # ------------------------------------------------------------------ the pass
    @torch.no_grad()
    def run(self, real, fake_rows, audio=None, alpha=None, on_grads=None, fake_ready=None):
        """real: (B, T, C) poses [any view of B*T*C], fake_rows: (B*T, C) generator rows (no graph), audio:
        (B, 1, S) for the two-branch critic, alpha: (B, 1) or (B,) interpolation weights on the device.
        Sets p.grad of every critic parameter (they must be None on entry: the engines zero with set_to_none);
        on_grads: called whenever further gradients are in place (GradExchange.poll).
        fake_ready: event after which `fake_rows` is complete (a generator forward still running on its own stream):
        only the pose branch waits for it - the audio branch's forward does not read the poses and starts at once.
        -> {"loss_critic", "gp", "w_dist"} (0-dim device tensors).

        Row layout of the pose branch. Piecewise-linear heads ('id', 'relu'): 3B rows [interpolated | real | fake];
        the penalty's tangent is written IN PLACE over the interpolated rows of the saved activations. `tanh` heads:
        4B rows, activation side [tangent | interpolated | real | fake], gradient side [first backward of the
        interpolated rows | the tanh'' chain | real | fake] - row r of one side pairs with row r of the other in the
        weight-gradient launches (see the module docstring)."""
        k = K()
        pose, au = self.pose, self.audio
        dev, dt = fake_rows.device, fake_rows.dtype
        C, CH, Cc = pose.C, pose.CH, pose.Cc
        Ca = au.Ca if au is not None else 0
        E = Cc + Ca
        B = real.size(0)
        T = real.numel() // (B * C)
        tanh = self.tanh
        i0 = B if tanh else 0                 # first forward row
        R = i0 + 3 * B
        fw, itp, tg = slice(i0, R), slice(i0, i0 + B), slice(0, B)   # forward rows, interpolated rows, tangent rows
        c1, cw, gamma_t = _cotangents(self._const, B, dev, dt, self.gamma, tanh)
        grads = _Grads(on_grads)

        # ---------------------------------------------------------------- forward: pose rows | audio, code rows
        side, cur = self._fork(dev)
        if fake_ready is not None:
            self._wait_for(fake_ready, fake_rows, side if side is not None else torch.cuda.current_stream(dev))
        with _on(side):
            X = torch.empty((R, C, T), dtype=dt, device=dev)
            k.pose_pack3(real.reshape(B, T, C), fake_rows, alpha.reshape(B), out=X[fw])
            a, p, q = pose.forward(X, fw)
            if tanh:
                # the activation masks of the interpolated rows, once more in the tangent block: the first backward then
                # runs as one launch per layer over all 4B rows with row-aligned masks (the tangent pass overwrites
                # a / p afterwards; q stays - it masks the interpolated rows' gradients in the weight-gradient launches)
                for t_ in a + p + q:
                    t_[tg].copy_(t_[itp])
        e = torch.empty((R, E), dtype=dt, device=dev)   # the code rows [pose code | audio code]
        ef = e[fw]
        if au is not None:
            au.forward(audio)
            if tanh:
                ea = k.tanh_fwd(k.gemm_ld(0, au.flat(au.hi), au.w6, au.l6[1], ACT_NONE))   # (B, Ca)
                ef.view(3, B, E)[:, :, Cc:] = ea
            else:
                k.gemm_ld(0, au.flat(au.hi), au.w6, au.l6[1], self.head_act, out=ef[0:B, Cc:])
                ef.view(3, B, E)[1:, :, Cc:] = ef[0:B, Cc:]
        with _on(side):
            if tanh:
                es = k.tanh_fwd(k.gemm_ld(0, a[-1][fw].view(3 * B, CH * T), pose.fw2d, pose.fconv[1], ACT_NONE))  # (3B, Cc)
                ef[:, :Cc] = es
            else:
                k.gemm_ld(0, a[-1].view(R, CH * T), pose.fw2d, pose.fconv[1], self.head_act, out=e[:, :Cc])
        self._join(side, cur, e)
        if tanh:
            e[tg] = e[itp]   # (gradient-side alignment, as for the masks above; the head's tangent lands here later)
        self._note(fw, X3=X, e=e, a=a, p=p, q=q)

        # ---------------------------------------------------------------- head forward + first backward
        if self.has_head:
            fc1, fc2 = self.critic.fc1, self.critic.fc2
            z = torch.empty((R, fc1.weight.shape[0]), dtype=dt, device=dev)
            k.gemm(0, ef, fc1.weight, fc1.bias, ACT_RELU, out=z[fw])
            s = k.gemm(0, z[fw], fc2.weight, fc2.bias)
            if tanh:
                z[tg] = z[itp]
            dzp = k.gemm(1, cw, fc2.weight, out_mask=z)            # (R, 128), multiplied by relu'(z); tanh: rows [B, 2B) = 0
            de_s = k.gemm_ld(1, dzp, fc1.weight[:, :Cc])           # (R, Cc)
            de_a = k.gemm_ld(1, dzp, fc1.weight[:, Cc:]) if au is not None else None
        else:
            s, dzp, de_s, de_a = e, None, c1, None
        if self.head_act == ACT_RELU:
            de_s = de_s * (e[:, :Cc] > 0)
            if de_a is not None:
                de_a = de_a * (e[:, Cc:] > 0)
        elif tanh:
            # through tanh: cotangent (1 - e^2); the raw cotangents of the interpolated rows are kept for the tanh'' term
            c_s_raw = de_s[tg].contiguous()
            de_s = k.tanh_bwd(de_s, e[:, :Cc].contiguous())
            if de_a is not None:
                c_a_raw = de_a[tg].contiguous()
                de_a = k.tanh_bwd(de_a, e[:, Cc:].contiguous())

        # ---------------------------------------------------------------- backward-data chains, penalties
        side, cur = self._fork(dev)
        with _on(side):
            da, dp = pose.backward_data(de_s)
            v_pose = pose.input_grad(tg)
            pen_p, norms_p = k.gp_penalty_fwd(v_pose.view(B, -1), self.lp)
        v_audio = pen_a = None
        if au is not None:
            au.seed(de_a[0:B], de_a[R - 2 * B:R - B], de_a[R - B:])
            if tanh:
                au.chain(au.lo)   # (the score half: after the tangent pass - the tanh'' cotangent joins it)
            elif self.merge_audio_chains:
                au.chain(None)
            else:
                au.chain(au.lo)
                au.chain(au.hi)
            v_audio = au.input_grad()
            pen_a, norms_a = k.gp_penalty_fwd(v_audio.view(B, -1), False)
        self._join(side, cur, pen_p, v_pose)
        self._note(slice(None), s=s, de_s=de_s, v_pose=v_pose, da=da, dp=dp, dzp=dzp)

        # ---------------------------------------------------------------- loss scalars, tangents
        losses = k.wgan_critic_loss(s.view(-1), B, pen_p, pen_a, self.gamma)
        side, cur = self._fork(dev)
        with _on(side):
            # G = gamma * d pen / d v over the tangent rows of X (in place for 3B layouts: those poses are not read again)
            k.gp_penalty_bwd(v_pose.view(B, -1), norms_p, gamma_t, self.lp, out=X[tg].view(B, -1))
            pose.tangent(tg, itp)
            if self.has_head and tanh:
                # tangent at u, then (a) through tanh into the head's code rows, (b) the tanh'' cotangent
                # w = t_u tanh''(u) c = tanh_bwd(tanh_bwd_bwd(t_u, c, e), e), which travels down the branch as an
                # ordinary gradient of the INTERPOLATED rows (gradient-side rows [B, 2B))
                t_u = k.gemm_ld(0, a[-1][tg].view(B, CH * T), pose.fw2d)
                e_i = es[0:B].contiguous()
                e[tg, :Cc] = k.tanh_bwd(t_u, e_i)
                de_s[itp] = k.tanh_bwd(k.tanh_bwd_bwd(t_u, c_s_raw, e_i), e_i)
                pose.backward_data(de_s, itp)
            elif self.has_head:
                hm = e[tg, :Cc] if self.head_act == ACT_RELU else None
                k.gemm_ld(0, a[-1][tg].view(B, CH * T), pose.fw2d, out_mask=hm, out=e[tg, :Cc])
        if au is not None:
            au.tangent(k.gp_penalty_bwd(v_audio.view(B, -1), norms_a, gamma_t, False).view(audio.shape))
            if tanh:
                t_ua = k.gemm_ld(0, au.flat(au.lo), au.w6)
                e[tg, Cc:] = k.tanh_bwd(t_ua, ea)
                au.ca2[au.hi] += k.tanh_bwd(k.tanh_bwd_bwd(t_ua, c_a_raw, ea), ea)
                au.chain(au.hi)
            else:
                hm = e[tg, Cc:] if self.head_act == ACT_RELU else None
                k.gemm_ld(0, au.flat(au.lo), au.w6, out_mask=hm, out=e[tg, Cc:])
        self._join(side, cur, e)
        self._note(tg, G0=X, ga=a, gp=p)
        if self.has_head:
            # tangent of the head: gz = relu'(z) * (W1 ge), in place over z's tangent rows (they hold the interpolated
            # rows' z: the mask)
            k.gemm(0, e[tg], fc1.weight, out_mask=z[tg], out=z[tg])

        # ---------------------------------------------------------------- weight gradients: one launch per layer
        # in REVERSE parameter order (head, audio branch from its last layer down, pose branch likewise; _Grads)
        side, cur = self._fork(dev)
        with _on(side):
            # (phase 2: the full-length conv IS the score; its rows pair (tangent, 1) / (activation, +-1/B))
            pose.weight_grads(de_s if self.has_head else c1, B, grads, defer=side is not None)
        if self.has_head:
            grads.put(fc2.weight, fc2.bias, k.gemm(2, cw, z), k.channel_sums(cw[B:].contiguous()))
            grads.put(fc1.weight, fc1.bias, k.gemm(2, dzp, e), k.channel_sums(dzp[B:].contiguous()))
        if au is not None:
            au.weight_grads(grads)
        self._join(side, cur, *[g for _, g in grads.late])
        grads.bind_late()
        grads.ready()
        pose.release()
        if au is not None:
            au.release()
        return {"loss_critic": losses[0], "gp": losses[1], "w_dist": losses[2]}


class GanCriticStep:
    """The critic iteration of the phase-2 `gan` framework (phase2/train.py:214-220) as one hand-scheduled pass:
    err_critic = BCE(critic(real), 1) + BCE(critic(fake), 0), no penalty, so no interpolated rows and no tangent.

      forward        pose branch ONCE over 2B rows [real | fake], channels-first; the full-length conv gives the 2B
                     scores (the phase-2 critic has no BatchNorm and no dropout: one pass equals two calls).
      loss           m2d_bce_logits_fwd writes the loss scalars AND the 2B score cotangents (sigmoid(s) - t) / B.
      backward-data  the chain of PoseBranch over the 2B rows.
      weight grads   one launch per layer over the 2B rows (PoseBranch's), every row an ordinary one.
    """

    @staticmethod
    def supports(critic):
        return (CriticStep.supports(critic) and not hasattr(critic, "fc1") and getattr(critic, "audio_d", None) is None
                and not getattr(critic, "_head_tanh", False) and int(getattr(critic, "_head_act", ACT_NONE)) == ACT_NONE)

    def __init__(self, critic):
        assert GanCriticStep.supports(critic)
        self.pose = PoseBranch(critic)

    @torch.no_grad()
    def run(self, real, fake_rows, on_grads=None):
        """real: (B, T, C) poses [any view of B*T*C], fake_rows: (B*T, C) generator rows (no graph). Sets p.grad of every
        critic parameter (None on entry). -> {"loss_critic", "err_real", "err_fake"} (0-dim device tensors)."""
        k = K()
        pose = self.pose
        C = pose.C
        B = real.size(0)
        T = real.numel() // (B * C)
        R = 2 * B
        X = torch.empty((R, C, T), dtype=fake_rows.dtype, device=fake_rows.device)
        X[:B].copy_(real.reshape(B, T, C).transpose(1, 2))
        X[B:].copy_(fake_rows.view(B, T, C).transpose(1, 2))
        a, _, _ = pose.forward(X, slice(0, R))
        s = k.gemm_ld(0, a[-1].view(R, pose.CH * T), pose.fw2d, pose.fconv[1], ACT_NONE)  # (2B, 1)
        losses, de_s = k.bce_logits_fwd(s.view(R), B, 1.0, B, 0.0, with_dx=True)
        de_s = de_s.view(R, 1)
        pose.backward_data(de_s)
        pose.weight_grads(de_s, 0, _Grads(on_grads))
        pose.release()
        return {"loss_critic": losses[0], "err_real": losses[1], "err_fake": losses[2]}


class CondCriticStep:
    """The critic iteration of the conditional phase-2 WGAN-LP (train_conditional.py:109-140 with the archis of
    phase2/archis/conditional.py) as one hand-scheduled pass:
    err_critic = mean(D(fake, fake_lbl)) - mean(D(real, real_lbl)) + gamma * LP, the interpolates scored with the REAL
    labels, LP = mean max(0, ||d D / d poses|| - 1)^2.

      forward        pose branch once over 3B rows [interpolated | real | fake], (69 + 4) channels each:
                     m2d_pose_pack3_label writes the poses and the label channels; the dropout mask (3B, CH, T) of
                     the three critic calls multiplies the full-length conv's input.
      backward-data  PoseBranch's chain, the mask applied to the full-length conv's input gradient; conv1's
                     backward-data runs over all 3B rows in one launch: rows [0, B) give the penalty's input gradient,
                     whose norm covers the 69 POSE channels only, rows [B, 3B) the label channels' gradient.
      embedding      dE from the real (cotangent -1/B) and fake (+1/B) rows only (m2d_label_embed_bwd): E reaches the
                     penalty through ReLU masks alone, so its penalty derivative is exactly zero.
      tangent        the penalty's tangent over the interpolated rows with ZERO label channels (conv1's second-order
                     weight-gradient term has no label-channel part), the mask applied at the full-length conv.
      weight grads   PoseBranch's pairing; the full-length conv pairs with the masked rows.
    """

    @staticmethod
    def supports(critic):
        return (hasattr(critic, "embed_label") and hasattr(critic, "dropout") and CriticStep.supports(critic)
                and not hasattr(critic, "fc1") and getattr(critic, "audio_d", None) is None
                and not getattr(critic, "_head_tanh", False) and int(getattr(critic, "_head_act", ACT_NONE)) == ACT_NONE)

    def __init__(self, critic, gamma, lp=True):
        assert CondCriticStep.supports(critic)
        self.critic = critic
        self.gamma = float(gamma)
        self.lp = bool(lp)
        self.pose = PoseBranch(critic)
        self.keep_p = 1.0 - float(critic.dropout.p)
        self._const = {}

    @torch.no_grad()
    def run(self, real, fake_rows, real_lbl, fake_lbl, alpha, keep=None, on_grads=None):
        """real: (B, T, 69) poses [any view of B*T*69], fake_rows: (B*T, 69) generator rows (no graph), real_lbl /
        fake_lbl: (B,) int64, alpha: (B, 1) or (B,) interpolation weights, keep: the (3B, CH, T) uint8 keep mask of the
        [interpolated | real | fake] critic calls, or None: Philox bits made on the device in the forward's dropout
        launch. Sets p.grad of every critic parameter (None on entry). -> {"loss_critic", "gp", "w_dist"}."""
        k = K()
        pose = self.pose
        dev, dt = fake_rows.device, fake_rows.dtype
        E = self.critic.embed_label.weight
        L, D = E.shape
        C = pose.C - D
        CH = pose.CH
        B = real.size(0)
        T = real.numel() // (B * C)
        R = 3 * B
        tg = slice(0, B)
        c1, _, gamma_t = _cotangents(self._const, B, dev, dt, self.gamma)
        sp = dict(p_keep=self.keep_p, scale=1.0 / self.keep_p)
        grads = _Grads(on_grads)

        # ---------------------------------------------------------------- forward
        X = k.pose_pack3_label(real.reshape(B, T, C), fake_rows, alpha.reshape(B), E, real_lbl, fake_lbl)
        a, _, _ = pose.forward(X, slice(0, R))
        if keep is None:
            seed, off = ops.philox_next()
            keep = torch.empty((R, CH, T), dtype=torch.uint8, device=dev)
            h = k.dropout(a[-1], keep, seed=seed, offset=off, **sp)
        else:
            h = k.dropout(a[-1], keep, **sp)
        s = k.gemm_ld(0, h.view(R, CH * T), pose.fw2d, pose.fconv[1], ACT_NONE)   # (3B, 1)

        # ---------------------------------------------------------------- backward-data, penalty, embedding
        pose.backward_data(c1, head=lambda g: k.dropout(g, keep, **sp))
        dX = pose.input_grad()                                                 # (3B, 69 + 4, T)
        v_pose = dX[tg, :C].contiguous()
        pen, norms = k.gp_penalty_fwd(v_pose.view(B, -1), self.lp)
        lbl2 = torch.cat((real_lbl, fake_lbl))
        dE = k.label_embed_bwd(dX, lbl2, B, R, C, L, D, 1)
        losses = k.wgan_critic_loss(s.view(-1), B, pen, None, self.gamma)

        # ---------------------------------------------------------------- tangent (label channels zero)
        X[tg, C:].zero_()
        X[tg, :C] = k.gp_penalty_bwd(v_pose.view(B, -1), norms, gamma_t, self.lp).view(B, C, T)
        pose.tangent(tg, tg)
        k.dropout(a[-1][tg], keep[tg], out=h[tg], **sp)

        # ---------------------------------------------------------------- weight gradients
        pose.weight_grads(c1, B, grads, head_in=h)
        E.grad = dE
        grads.ready()
        pose.release()
        return {"loss_critic": losses[0], "gp": losses[1], "w_dist": losses[2]}
