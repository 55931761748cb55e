"""Launch traces of the hand-scheduled critic iterations (music2dance_amd/critic_step.py): the recorder, the cases and
the recorded files tests/test_critic_step_trace.py pins. A helper, not a test module.

A trace is what one `run` of a critic step asks of the layers below it, one line per entry, in order:

  k <method>(...) -> ...    a call of a kernel wrapper (kernels.impl()): every scalar argument by value, every tensor
                            argument as t<storage>+<offset>:<shape>/<strides> - <storage> the ordinal of the tensor's
                            storage by first appearance in the trace, so two views of one buffer (the tangent written
                            over the interpolated rows, an `out=` block of a wider buffer) show as the same ordinal -
                            and the result likewise.
  a <op> <shapes>           an ATen operator the schedule issues itself, between wrapper calls (what the wrappers issue
                            inside is theirs, not the schedule's). Views, metadata and `empty*` are left out: they
                            launch nothing.
  on_grads bound=<n>        a call of `on_grads`, with the number of parameters whose .grad is bound at that point.

With streams=True (the GPU cases) every entry ends in `@side` when the current stream is the critic's pose-branch
stream, and `wait_stream`, `wait_event` and `record_stream` calls are entries of their own (`s ...`): the fork, join
and lifetime edges of the schedule.

The files under tests/critic_traces/ were recorded by `python -m tests.critic_trace --record` (CPU cases, stand-in
kernels of tests/fake_backend.py) and `--record --gpu` (real kernels, MI355X) from the commit BEFORE critic_step.py
was split into a schedule and two branch objects, with only these test files added. The expectations are therefore
never the output of the code under test. Record again ONLY when the launch list is changed on purpose, from the commit
before that change plus the reviewed differences.
"""
import contextlib
import os

import torch
from torch.utils._python_dispatch import TorchDispatchMode

from music2dance_amd import kernels
from music2dance_amd.critic_step import CondCriticStep, CriticStep, GanCriticStep

TRACE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "critic_traces")
_SKIP_ATEN = ("aten.empty", "aten._unsafe_view", "aten.detach", "aten.alias", "aten.lift_fresh", "aten.sym_",
              "aten.record_stream")


def _is_view(func):
    """a pure view: a result aliases an argument that is not written"""
    return any(r.alias_info is not None and not r.alias_info.is_write for r in func._schema.returns)


class Recorder:
    """Wraps a kernel layer (anything kernels.impl() may return); .lines is the trace."""

    def __init__(self, inner, streams=False, side=lambda: None):
        self._inner = inner
        self._streams = streams
        self._side = side          # -> the pose-branch stream (it exists only after the first fork)
        self._storages = {}        # StorageImpl -> ordinal; the storages are held, so an address is never reused
        self._held = []
        self._depth = 0            # > 0: inside a wrapper call (its ATen ops are not the schedule's)
        self.lines = []

    # ------------------------------------------------------------------ formatting
    def _tensor(self, t):
        st = t.untyped_storage()
        key = st._cdata
        if key not in self._storages:
            self._storages[key] = len(self._storages)
            self._held.append(st)
        dt = "" if t.dtype == torch.float32 else ":" + str(t.dtype).replace("torch.", "")
        return "t%d+%d:%s/%s%s" % (self._storages[key], t.storage_offset(), ",".join(map(str, t.shape)),
                                   ",".join(map(str, t.stride())), dt)

    def _value(self, v):
        if isinstance(v, torch.Tensor):
            return self._tensor(v)
        if isinstance(v, (tuple, list)):
            return "(" + " ".join(self._value(x) for x in v) + ")"
        if isinstance(v, float):
            return "%.9g" % v
        return repr(v)

    def stream_name(self, s):
        side = self._side()
        if side is not None and s == side:
            return "side"
        return "main" if s == torch.cuda.default_stream(s.device) else "other"

    def log(self, text):
        if self._streams and self._side() is not None and torch.cuda.current_stream() == self._side():
            text += " @side"
        self.lines.append(text)

    # ------------------------------------------------------------------ the kernel layer
    def __getattr__(self, name):
        fn = getattr(self._inner, name)
        if not callable(fn):
            return fn

        def call(*args, **kwargs):
            if self._depth:
                return fn(*args, **kwargs)
            parts = [self._value(a) for a in args] + ["%s=%s" % (k, self._value(v)) for k, v in kwargs.items()]
            self._depth += 1
            try:
                out = fn(*args, **kwargs)
            finally:
                self._depth -= 1
            self.log("k %s(%s) -> %s" % (name, " ".join(parts), self._value(out)))
            return out

        return call

    # ------------------------------------------------------------------ ATen ops, on_grads, stream edges
    def aten_mode(self):
        rec = self

        class Mode(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                out = func(*args, **(kwargs or {}))
                name = str(func)
                if not rec._depth and not name.startswith(_SKIP_ATEN) and not _is_view(func):
                    shapes = [",".join(map(str, a.shape)) or "-" for a in list(args) + list((kwargs or {}).values())
                              if isinstance(a, torch.Tensor)]
                    rec.log(" ".join(["a", name] + shapes))
                return out

        return Mode()

    def on_grads(self, params):
        params = list(params)
        return lambda: self.log("on_grads bound=%d" % sum(p.grad is not None for p in params))

    @contextlib.contextmanager
    def stream_edges(self):
        """wait_stream / wait_event / record_stream as entries (torch.cuda.Stream and torch.Tensor patched meanwhile)"""
        S, T = torch.cuda.Stream, torch.Tensor
        saved = S.wait_stream, S.wait_event, T.record_stream
        rec = self

        def wait_stream(self, other):
            rec.log("s wait_stream %s <- %s" % (rec.stream_name(self), rec.stream_name(other)))
            return saved[0](self, other)

        def wait_event(self, event):
            rec.log("s wait_event %s" % rec.stream_name(self))
            return saved[1](self, event)

        def record_stream(self, stream):
            if not rec._depth:
                rec.log("s record_stream %s on %s" % (rec._tensor(self), rec.stream_name(stream)))
            return saved[2](self, stream)

        S.wait_stream, S.wait_event, T.record_stream = wait_stream, wait_event, record_stream
        try:
            yield
        finally:
            S.wait_stream, S.wait_event, T.record_stream = saved


# ---------------------------------------------------------------------------------------------------- the cases
def _inputs(B, T, dev, audio, seed=3):
    """(tests/test_critic_step.py: _inputs)"""
    g = torch.Generator().manual_seed(seed)
    real = torch.rand(B, T, 69, generator=g).to(dev)
    fake_rows = (torch.rand(B * T, 69, generator=g) * 1.5 - 0.2).to(dev)
    alpha = torch.rand(B, 1, generator=g).to(dev)
    aud = (0.1 * torch.randn(B, 1, 640 * T, generator=g)).to(dev) if audio else None
    return real, fake_rows, alpha, aud


def _two_branch(activ, merge=True, event=False):
    def make(dev):
        from music2dance_amd.phase3.archis import default as p3
        torch.manual_seed(0)
        critic = p3.SequenceDiscriminator(69, 16, 12, 120, init_ker=25, activ=activ, device="cpu").to(dev)
        real, fake_rows, alpha, audio = _inputs(2, 120, dev, True)
        step = CriticStep(critic, 10.0, lp=False)
        step.merge_audio_chains = merge
        kw = {}
        if event:
            # the generator forward's stand-in: the rows are complete after an event on a stream of their own
            gen = torch.cuda.Stream(dev)
            gen.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(gen):
                fake_rows = fake_rows.clone()
                kw["fake_ready"] = gen.record_event()
        return critic, step, (real, fake_rows, audio, alpha), kw
    return make


def _ablated(activ):
    def make(dev):
        from music2dance_amd.phase3.archis import default as p3
        torch.manual_seed(1)
        critic = p3.AblatedSequenceDiscriminator(69, 16, 12, 40, init_ker=25, activ=activ, device="cpu").to(dev)
        real, fake_rows, alpha, _ = _inputs(3, 40, dev, False)
        return critic, CriticStep(critic, 10.0, lp=False), (real, fake_rows, None, alpha), {}
    return make


def _phase2(lp, n_blocks=3):
    def make(dev):
        from music2dance_amd.phase2.archis import default as p2
        torch.manual_seed(2)
        critic = p2.SequenceDiscriminator(69, 16, 30, 25, n_blocks, "cpu").to(dev)
        real, fake_rows, alpha, _ = _inputs(4, 30, dev, False)
        return critic, CriticStep(critic, 10.0, lp=lp), (real, fake_rows, None, alpha), {}
    return make


def _gan(dev):
    from tests.test_p2_gan_host import B, T, _make_p2
    _, critic = _make_p2()
    real = torch.rand(B, T, 69, generator=torch.Generator().manual_seed(4))
    fake_rows = torch.rand(B * T, 69, generator=torch.Generator().manual_seed(5))
    return critic, GanCriticStep(critic), (real, fake_rows), {}


def _cond(given_keep):
    def make(dev):
        from music2dance_amd import ops
        from music2dance_amd.phase2.archis.conditional import SequenceDiscriminator
        torch.manual_seed(0)
        critic = SequenceDiscriminator(69, 8, 24, 5, 1)
        g = torch.Generator().manual_seed(4)
        real = torch.rand(3, 24, 69, generator=g)
        fake_rows = torch.rand(3 * 24, 69, generator=g)
        alpha = torch.rand(3, 1, generator=g)
        keep = (torch.rand(9, 8, 24, generator=g) < 0.5).to(torch.uint8) if given_keep else None
        torch.manual_seed(11)   # (keep=None: the Philox seed is torch's, the offset counts the masks of this process)
        ops._PHILOX["offset"] = 0
        return (critic, CondCriticStep(critic, 10.0, lp=True),
                (real, fake_rows, torch.tensor([0, 3, 3]), torch.tensor([1, 1, 2]), alpha), {"keep": keep})
    return make


def _fake(kind):
    def make():
        if kind == "gan":
            from tests.test_p2_gan_host import BceFakeKernels
            return BceFakeKernels()
        if kind == "cond":
            from tests.test_p2_cond_host import CondFakeKernels
            return CondFakeKernels()
        from tests.fake_backend import FakeKernels
        return FakeKernels()
    return make


# name -> (case builder, stand-in kernel layer): every branch of the three run() methods
CPU_CASES = {
    "two_branch_id": (_two_branch("id"), _fake("p3")),
    "two_branch_relu": (_two_branch("relu"), _fake("p3")),
    "two_branch_tanh": (_two_branch("tanh"), _fake("p3")),
    "two_branch_id_unmerged": (_two_branch("id", merge=False), _fake("p3")),
    "ablated_id": (_ablated("id"), _fake("p3")),
    "ablated_tanh": (_ablated("tanh"), _fake("p3")),
    "phase2_lp": (_phase2(True), _fake("p3")),
    "phase2_gp": (_phase2(False), _fake("p3")),
    "phase2_no_blocks": (_phase2(True, n_blocks=0), _fake("p3")),
    "gan": (_gan, _fake("gan")),
    "cond_keep": (_cond(True), _fake("cond")),
    "cond_philox": (_cond(False), _fake("cond")),
}
# the real kernels with streams: the two-branch critic, with and without an event the pose branch has to wait for
GPU_CASES = {
    "gpu_two_branch_id": _two_branch("id"),
    "gpu_two_branch_tanh": _two_branch("tanh"),
    "gpu_two_branch_id_event": _two_branch("id", event=True),
    "gpu_two_branch_tanh_event": _two_branch("tanh", event=True),
}


def trace(name):
    """-> the trace of case `name`, a list of lines"""
    gpu = name in GPU_CASES
    if gpu:
        make, dev, inner = GPU_CASES[name], torch.device("cuda:0"), kernels.impl()
        assert inner.name == "hip"
    else:
        make, dev, inner = CPU_CASES[name][0], torch.device("cpu"), CPU_CASES[name][1]()
    prev = kernels.set_impl(inner)   # (the case builders construct networks: they may ask the kernel layer)
    try:
        critic, step, args, kw = make(dev)
        for p in critic.parameters():
            p.grad = None
        rec = Recorder(inner, streams=gpu, side=lambda: getattr(critic, "_stick_stream", None))
        kernels.set_impl(rec)
        with contextlib.ExitStack() as stack:
            if gpu:
                torch.cuda.synchronize()
                stack.enter_context(rec.stream_edges())
            stack.enter_context(rec.aten_mode())
            step.run(*args, on_grads=rec.on_grads(critic.parameters()), **kw)
        if gpu:
            torch.cuda.synchronize()
        assert all(p.grad is not None for p in critic.parameters())
        return rec.lines
    finally:
        kernels.set_impl(prev)


def recorded(name):
    with open(os.path.join(TRACE_DIR, name + ".txt")) as f:
        return f.read().splitlines()


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--record", action="store_true", help="write the traces (see the module docstring for WHEN)")
    ap.add_argument("--gpu", action="store_true", help="the GPU cases (real kernels) instead of the CPU ones")
    ap.add_argument("--out", default=TRACE_DIR)
    a = ap.parse_args(argv)
    os.makedirs(a.out, exist_ok=True)
    for name in (GPU_CASES if a.gpu else CPU_CASES):
        lines = trace(name)
        again = trace(name)
        assert lines == again, "%s: the trace differs run to run" % name
        print("%-28s %4d entries" % (name, len(lines)))
        if a.record:
            with open(os.path.join(a.out, name + ".txt"), "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
