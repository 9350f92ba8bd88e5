"""Per-rank closed-loop fleet driver: the loop bench.py times on every GPU.

One step of a fleet of kites on one rank:

  [EKF]  estimator (kiteEKF.cpp:75-126, BASELINE configs[4]): propagate the
         estimate under the control applied last, in `ekf_substeps` RK4 steps
         of dt/ekf_substeps, and update it with the measured position +
         attitude (z, 7 values) on the last one; the RTI starts from the
         estimate.  With ``wind_ekf`` instead: the filter that carries the
         wind as three more states (kite_nmpc_windekf_step_device), the same
         propagation and update in one launch, after which the estimated wind
         becomes the wind of the RTI's model (kite_nmpc_set_wind_device).
         With ``kin_ekf``: the kinematic, model-free filter of the reference's
         estimator node (kite_nmpc_kinekf_step_device), one launch as well;
         it uses no control and no aerodynamic constant, so a flight log
         recorded from it is independent of every model row.
  RTI    one real-time iteration of the NMPC for every kite of the shard
         (kite_nmpc_step_device: KiteNMPF::computeControl, kiteNMPF.cpp:199-316).
  pub    optional publish of u0 + mpc_diagnostic of every kite to every rank
         (shard.Publisher: one all-gather, RCCL over xGMI / gloo on CPU).
  plant  closed loop on synthetic data (in episodes: ``restart`` puts every
         kite back at its launch state, see bench.py --episode): the next
         measured state is the plan's
         prediction at t0 + dt (trajectory node 1), and its position +
         attitude are the next EKF measurement.  With ``noise`` (a
         ``MeasurementNoise``) that state is disturbed before it is measured:
         the controller's model no longer predicts the plant exactly.
         With ``plant`` (a ``GpuPlant``) the kite is a simulator of its own:
         the loop carries the true 13 kite states and a time, advances them
         over dt under u(t0) with the plant's own parameters, wind and gust
         (kite_nmpc_plant_step_device), and measures that state; theta and
         thetadot still come from the plan's node 1 (nmpf_node.cpp:220).
         With ``GpuPlant(..., delay=ActuationDelay(...))`` u(t0) is sent down
         a per-kite command line (transport_delay.cpp) and the kite flies what
         has arrived (kite_nmpc_plant_step_delayed_device, still one launch);
         the estimators propagate under that control, ``restart`` resets the
         lines (fresh lines are empty schedules), and with ``delay_comp="queue"``
         the RTI's delay compensation predicts under the commands still in the
         line (kite_nmpc_set_inflight_device right before the step) instead of
         the last u(t0) alone; a ``recorder`` logs what flew (accepted only where it is constant
         over a period: no jitter, a mean of whole periods).

  adapt  with ``recorder`` and ``adapt`` (an ``IdentConfig``): each time the
         flight log is full, before the RTI, every kite's 21 aerodynamic
         coefficients are identified from it (kite_nmpc_identify_device) and
         become that kite's controller model (kite_nmpc_set_params_device),
         all on the stream.  With ``estimator_model="controller"`` the
         estimator filters with those models too (kite_nmpc_set_estimator_model),
         from the step after the identification on; the default keeps the
         creation model in the filter.  With ``ident_wind`` (and a
         ``FlightRecorder(..., wind=True)``) the wind of each period is logged
         next to the control -- a known (B, 3) wind, or with ``"estimate"`` the
         wind EKF's estimate as the controller received it -- and the
         identification fits the model that sees it
         (kite_nmpc_identify_wind_device).

  score  with ``scorer`` (an ``EpisodeScore``): right after the RTI the period
         is scored on the stream (kite_nmpc_score_step_device, one launch): the
         true state at t0 (the plant's; without one the state the plan started
         from), the control just computed and the two status words go into
         per-kite accumulators -- the true cross-track error against the
         global closest point of the path, the controller's costs there, the
         control rate, the airspeed, the progress round the path, the lost
         periods.  ``restart`` marks the next period as an episode's first;
         the accumulators persist until ``scorer.reset()``.

The stepper does the arithmetic; ``GpuStepper`` drives libkite_nmpc.so on
device tensors.  Tests plug a CPU oracle stepper into the same loop to check
the sharded multi-rank flow against the unsharded batch.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch


class GpuStepper:
    """RTI + EKF of one C-ABI context on device tensors (asynchronous on the
    context stream; give the context torch's stream with ``set_stream``)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def rti(self, x0, u0, traj, diag, status):
        self.ctx.step_device(x0.data_ptr(), u0.data_ptr(), traj.data_ptr(), 0, diag.data_ptr(),
                             status.data_ptr())

    def reset(self):
        self.ctx.reset()

    def ekf(self, dt, xe, u3, P, z, W, V):
        self.ctx.ekf_step_device(xe.shape[0], dt, xe.data_ptr(), u3.data_ptr(), P.data_ptr(),
                                 z.data_ptr() if z is not None else 0, W.data_ptr(), V.data_ptr())

    def wind_ekf(self, dt, substeps, xe, u3, P, z, W, V, status):
        """One fused step of the wind-estimating EKF on xe (B, 16) and P (B, 16, 16)."""
        self.ctx.wind_ekf_step_device(xe.shape[0], dt, substeps, xe.data_ptr(), u3.data_ptr(), P.data_ptr(),
                                      z.data_ptr() if z is not None else 0, W.data_ptr(), V.data_ptr(),
                                      status.data_ptr() if status is not None else 0)

    def kin_ekf(self, dt, substeps, xe, P, z, W, V, status, frame=None):
        """One fused step of the kinematic EKF on xe (B, 13) and P (B, 13, 13);
        frame: a ``PoseFrame`` when z holds motion-capture poses."""
        self.ctx.kin_ekf_step_device(xe.shape[0], dt, substeps, xe.data_ptr(), P.data_ptr(),
                                     z.data_ptr() if z is not None else 0, W.data_ptr(), V.data_ptr(),
                                     status.data_ptr() if status is not None else 0, frame=frame)

    def set_wind_device(self, wind, wmax):
        """The controller's wind from a (B, 3) view of a device tensor (rows
        ``wind.stride(0)`` doubles apart, components contiguous)."""
        assert wind.dtype == torch.float64 and wind.stride(1) == 1
        self.ctx.set_wind_device(wind.data_ptr(), wind.stride(0), wmax)

    def set_inflight_device(self, line, t0):
        """The delay compensation's in-flight schedule from the kites' command
        lines, a contiguous (B, DELAY_NLINE) device tensor, as they stand at
        time t0 (kite_nmpc_set_inflight_device); None switches it off."""
        if line is None:
            self.ctx.set_inflight_device(0, t0)
            return
        assert line.dtype == torch.float64 and line.is_contiguous()
        self.ctx.set_inflight_device(line.data_ptr(), t0)

    def set_params_device(self, rows, status=None):
        """The controller's per-kite models from a contiguous (B, 52) device
        tensor of kite_params rows; status (B,) int32 receives the
        KITE_PARAMS_* words."""
        assert rows.dtype == torch.float64 and rows.is_contiguous() and rows.shape[1] == 52
        self.ctx.set_params_device(rows.data_ptr(), rows.shape[0], status.data_ptr() if status is not None else 0)

    def set_estimator_model(self, mode: int):
        """The model of the stepper's EKFs (``BatchNMPC.set_estimator_model``)."""
        self.ctx.set_estimator_model(mode)

    def get_params(self):
        """The (B, 52) rows in force, on the host."""
        return self.ctx.get_params()

    def identify(self, config, T, rows, X, U, out, cost2, evals, status, ws, W=None):
        """kite_nmpc_identify_device on device tensors, a row per kite; W: the
        wind log (B, T, 3) (kite_nmpc_identify_wind_device), None: windless."""
        self.ctx.identify_device(config, rows.shape[0], T, rows.data_ptr(), rows.shape[0], X.data_ptr(), U.data_ptr(),
                                 out.data_ptr(), cost2.data_ptr(), evals.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                 wind=W.data_ptr() if W is not None else 0)

    def identify_joint(self, config, wind_config, T, rows, X, U, out, wind_out, cost2, evals, status, ws, W0=None):
        """kite_nmpc_identify_joint_device on device tensors, a row per kite: the
        21 and a constant wind offset (wind_out (B, 3)); W0: a known wind log
        (B, T, 3) the offset is added to, None: zeros."""
        self.ctx.identify_joint_device(config, wind_config, rows.shape[0], T, rows.data_ptr(), rows.shape[0],
                                       X.data_ptr(), U.data_ptr(), out.data_ptr(), wind_out.data_ptr(),
                                       cost2.data_ptr(), evals.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                       wind0=W0.data_ptr() if W0 is not None else 0)

    def score(self, x13, u4, status, plant_status, first, acc, mem):
        """One control period of every kite into the accumulators acc (B, 16) and
        mem (B, 8), one launch on the stream (kite_nmpc_score_step_device); x13
        (B, 13) and u4 (B, 4) contiguous, status / plant_status (B,) int32 or None."""
        assert x13.dtype == torch.float64 and x13.is_contiguous() and u4.is_contiguous()
        self.ctx.score_step_device(x13.shape[0], x13.data_ptr(), u4.data_ptr(),
                                   status.data_ptr() if status is not None else 0,
                                   plant_status.data_ptr() if plant_status is not None else 0, first,
                                   acc.data_ptr(), mem.data_ptr())

    def score_summary(self, acc, out):
        """out (16,) <- the raw fleet summary of acc (B, 16), on the stream."""
        self.ctx.score_summary_device(acc.shape[0], acc.data_ptr(), out.data_ptr())


class EpisodeScore:
    """Per-kite flight metrics of a fleet on the device, filled one launch per
    control period by ``FleetLoop(scorer=...)`` (or by ``GpuStepper.score``):
    acc (B, 16) the accumulator rows (slots ``nmpc.SCORE_*``), mem (B, 8) what
    a period needs of the one before, ``first`` the flag of the period that
    starts an episode.  The accumulators persist across episodes: ``reset``
    alone clears them.  Behind a delayed plant (``ActuationDelay``) the loop
    still scores the commanded u0 (control effort, control rate), not the
    line's control in force; the tracking figures see the delay through the
    true state.  Nothing here synchronises except ``summary``, which
    brings 16 doubles to the host."""

    def __init__(self, B: int, device=None):
        self.B = int(B)
        f64 = dict(dtype=torch.float64, device=device)
        self.acc = torch.zeros((self.B, 16), **f64)
        self.mem = torch.zeros((self.B, 8), **f64)
        self._sum = torch.zeros((16,), **f64)
        self.first = True
        self.stepper, self.dt = None, None         # set by the loop that scores into this

    def reset(self):
        self.acc.zero_()
        self.mem.zero_()
        self.first = True

    def rows(self) -> dict:
        """The accumulator rows by name, (B,) tensors each (views of acc)."""
        from . import nmpc
        return {name: self.acc[:, i] for i, name in enumerate(nmpc.SCORE_SLOTS)}

    def summary(self, stepper=None, dt: Optional[float] = None) -> dict:
        """The fleet summary: the raw 16 ("raw", a list: what ``combine`` takes)
        and the figures derived from them (``nmpc.score_derive``).  The
        reduction runs on ``stepper`` (default: the stepper and the dt of the
        loop this scorer was given to)."""
        from . import nmpc
        stepper = stepper if stepper is not None else self.stepper
        if stepper is None:
            raise ValueError("EpisodeScore.summary: no stepper (give one, or give the scorer to a FleetLoop)")
        dt = dt if dt is not None else self.dt
        stepper.score_summary(self.acc, self._sum)
        raw = self._sum.cpu().numpy().copy()
        out = nmpc.score_derive(raw, dt)
        out["raw"] = raw.tolist()
        return out

    @staticmethod
    def combine(raw_summaries, dt: Optional[float] = None) -> dict:
        """The summary of several ranks' raw summaries (gathered by any means):
        host arithmetic, no GPU."""
        from . import nmpc
        raw = nmpc.score_combine(raw_summaries)
        out = nmpc.score_derive(raw, dt)
        out["raw"] = raw.tolist()
        return out


class ActuationDelay:
    """The command line of every kite of a delayed plant (``GpuPlant(...,
    delay=)``, kite_nmpc_plant_step_delayed_device) on the device: ``line`` (B,
    DELAY_NLINE) the control in force and the FIFO of pending commands,
    ``u_applied`` (B, 4) the control in force during the last plant step of the
    last period, ``tau`` (B,) the latencies of the last send.  Each period
    ``draw`` takes tau uniform on [max(mean - deviation, 0), mean + deviation]
    (seconds; the reference's transport_delay node, there in ms) from a seeded
    device generator; deviation == 0 draws nothing, tau is the mean.  A command
    arrives at max(t_send, previous arrival) + tau (``rule="sequential"``, the
    default): a mean above the control period is a channel that falls behind
    and drops its oldest commands.  ``rule="transport"``: it arrives at
    max(t_send + tau, previous arrival), a pure transport delay that still
    never reorders; the rule is written into every line's ``DELAY_RULE`` slot."""

    RULES = {"sequential": 0.0, "transport": 1.0}      # nmpc.DELAY_RULE_*

    def __init__(self, B: int, mean: float, deviation: float = 0.0, seed: int = 0, device=None,
                 rule: str = "sequential"):
        from . import nmpc
        if not (mean >= 0.0 and math.isfinite(mean)) or not (deviation >= 0.0 and math.isfinite(deviation)):
            raise ValueError("ActuationDelay: mean and deviation are finite and >= 0")
        if rule not in self.RULES:
            raise ValueError('ActuationDelay: rule is "sequential" or "transport"')
        self.rule = rule
        f64 = dict(dtype=torch.float64, device=device)
        self.B, self.mean, self.deviation, self.seed = int(B), float(mean), float(deviation), int(seed)
        self.lo, self.hi = max(self.mean - self.deviation, 0.0), self.mean + self.deviation
        self.line = torch.zeros((self.B, nmpc.DELAY_NLINE), **f64)
        self.u_applied = torch.zeros((self.B, 4), **f64)
        self.tau = torch.full((self.B,), self.lo, **f64)
        self.gen = torch.Generator(device=self.line.device)
        self.gen.manual_seed(self.seed)
        self._rule_slot = nmpc.DELAY_RULE
        if self.RULES[rule] != 0.0:
            self.line[:, self._rule_slot] = self.RULES[rule]

    def reset(self):
        """Fresh lines (empty, zero control in force, the rule in its slot) and
        the generator back at its seed."""
        self.line.zero_()
        if self.RULES[self.rule] != 0.0:
            self.line[:, self._rule_slot] = self.RULES[self.rule]
        self.u_applied.zero_()
        self.gen.manual_seed(self.seed)

    def draw(self) -> torch.Tensor:
        """The latencies of this period's send, (B,)."""
        if self.hi > self.lo:
            r = torch.rand((self.B,), generator=self.gen, dtype=torch.float64, device=self.line.device)
            torch.add(r * (self.hi - self.lo), self.lo, out=self.tau)
        return self.tau


class GpuPlant:
    """The batched plant simulator of one C-ABI context on device tensors
    (kite_nmpc_plant_step_device: the context's plant parameters, wind and gust,
    see ``BatchNMPC.plant_set_params`` / ``plant_set_wind``): ``steps`` plant
    steps of ``h`` per control period, RK4 with ``substeps`` each.  With
    ``delay`` (an ``ActuationDelay``) the command goes through the kites' lines
    and the period is the one delayed launch; None: the undelayed call."""

    def __init__(self, ctx, h: float = 0.02, steps: int = 1, substeps: int = 4, delay=None):
        self.ctx, self.h, self.steps, self.substeps = ctx, float(h), int(steps), int(substeps)
        self.delay = delay

    def advance(self, x13, u0, t0, status):
        """x13 (B, 13) in place from t0 over steps * h under the held u0 (B, 4)
        -- with a delay: u0 is sent at t0 and the line decides what flies;
        status (B,) int32 receives the KITE_PLANT_* words."""
        d = self.delay
        if d is None:
            self.ctx.plant_step_device(x13.data_ptr(), u0.data_ptr(), t0, self.h, self.steps, self.substeps,
                                       status.data_ptr())
            return
        assert u0.is_contiguous() and x13.shape[0] == d.B
        self.ctx.plant_step_delayed_device(x13.data_ptr(), u0.data_ptr(), d.draw().data_ptr(), d.line.data_ptr(), t0,
                                           self.h, self.steps, self.substeps, d.u_applied.data_ptr(),
                                           status.data_ptr())


class FlightRecorder:
    """Flight log of a fleet on the device for the parameter identification
    (``BatchNMPC.identify_device``): X (B, T+1, 13) the kite state handed to the
    controller at the start of each control period, U (B, T, 3) the control
    (T, dE, dR) applied over it.  ``FleetLoop(recorder=...)`` fills it, one
    period per step, and it stops when full (``full``).  With ``wind=True`` it
    also owns W (B, T, 3), the known world-frame wind of each period
    (``record_wind``, next to ``record_control``), and ``identify`` fits the
    model that sees that wind (kite_nmpc_identify_wind_device)."""

    def __init__(self, B: int, T: int, device=None, wind: bool = False):
        f64 = dict(dtype=torch.float64, device=device)
        self.B, self.T = int(B), int(T)
        self.X = torch.zeros((self.B, self.T + 1, 13), **f64)
        self.U = torch.zeros((self.B, self.T, 3), **f64)
        self.W = torch.zeros((self.B, self.T, 3), **f64) if wind else None
        self.nx = 0            # states recorded
        self.nu = 0            # controls recorded

    @property
    def full(self) -> bool:
        return self.nx == self.T + 1 and self.nu == self.T

    def reset(self):
        self.nx = self.nu = 0

    def record_state(self, x0: torch.Tensor) -> None:
        if self.nx <= self.T:
            self.X[:, self.nx, :].copy_(x0[:, :13])
            self.nx += 1

    def record_wind(self, w3: torch.Tensor) -> None:
        """The wind (B, 3) of the period whose control comes next: row ``nu``,
        so call it before that period's ``record_control``."""
        if self.W is None:
            raise ValueError("the recorder logs no wind: FlightRecorder(..., wind=True)")
        if self.nu < self.T:
            self.W[:, self.nu, :].copy_(w3)

    def record_control(self, u0: torch.Tensor) -> None:
        if self.nu < self.T:
            self.U[:, self.nu, :].copy_(u0[:, :3])
            self.nu += 1

    def identify(self, ctx, config, params=None):
        """Identify every kite's 21 aerodynamic coefficients from the log
        (asynchronous on the context stream, as the loop's other calls).
        config: an ``IdentConfig``; for a loop flown against
        ``GpuPlant(h, steps, substeps)`` with control period dt = h * steps the
        model that repeats the plant's arithmetic is h = dt, substeps = steps *
        substeps.  params: the rows the fit starts from (52 values or (B, 52));
        None: the context's own.  Returns device tensors
        (params (B, 52), cost2 (B, 2), evals (B,), status (B,))."""
        from . import nmpc
        if not self.full:
            raise ValueError(f"the log holds {self.nx} of {self.T + 1} states")
        dev = self.X.device
        rows = torch.from_numpy(ctx._ident_rows(params, self.B).copy()).to(dev)
        out = torch.zeros((self.B, 52), dtype=torch.float64, device=dev)
        cost2 = torch.zeros((self.B, 2), dtype=torch.float64, device=dev)
        evals = torch.zeros((self.B,), dtype=torch.int32, device=dev)
        status = torch.zeros((self.B,), dtype=torch.int32, device=dev)
        ws = torch.empty((nmpc.ident_workspace_doubles(config, self.B, self.T),), dtype=torch.float64, device=dev)
        ctx.identify_device(config, self.B, self.T, rows.data_ptr(), rows.shape[0], self.X.data_ptr(),
                            self.U.data_ptr(), out.data_ptr(), cost2.data_ptr(), evals.data_ptr(), status.data_ptr(),
                            ws.data_ptr(), wind=self.W.data_ptr() if self.W is not None else 0)
        self._keep = (rows, ws)      # alive until the stream has run the launches
        return out, cost2, evals, status


class MeasurementNoise:
    """Seeded Gaussian disturbance of the measured kite state (bench.py
    --meas-noise): per step and kite, body velocity += 0.05 S, body rates +=
    0.05 S, position += 0.01 S (N(0, 1) draws, SI units), attitude rotated by
    a random small angle of about 0.01 S rad (quaternion renormalised);
    theta / thetadot are the controller's own states and stay untouched.  The
    draws come from a device generator seeded per rank, so a run is
    reproducible and the noise costs two small kernels per step."""

    SCALE = (0.05, 0.05, 0.01, 0.005)

    def __init__(self, sigma: float, device, seed: int):
        self.sigma = float(sigma)
        self.gen = torch.Generator(device=device)
        self.gen.manual_seed(int(seed))

    def apply(self, x: torch.Tensor) -> None:
        B = x.shape[0]
        n = torch.randn((B, 13), generator=self.gen, dtype=x.dtype, device=x.device)
        sv, sw, sr, sq = (self.sigma * c for c in self.SCALE)
        x[:, 0:3] += sv * n[:, 0:3]
        x[:, 3:6] += sw * n[:, 3:6]
        x[:, 6:9] += sr * n[:, 6:9]
        q = x[:, 9:13] + sq * n[:, 9:13]
        x[:, 9:13] = q / q.norm(dim=1, keepdim=True)


class FleetLoop:
    """Closed-loop state of one rank's shard and its per-step sequence."""

    def __init__(self, stepper, x0: torch.Tensor, N: int, dt: float, ekf: bool = False, ekf_substeps: int = 5,
                 covariances: Optional[tuple] = None, publisher=None, noise: Optional[MeasurementNoise] = None,
                 plant=None, wind_ekf: bool = False, wind_max: float = 20.0, recorder=None, adapt=None,
                 estimator_model: str = "creation", ident_wind=None, kin_ekf: bool = False,
                 ident_wind_config=None, scorer=None, delay_comp: str = "last"):
        if delay_comp not in ("last", "queue"):
            raise ValueError('delay_comp is "last" or "queue"')
        if delay_comp == "queue" and getattr(plant, "delay", None) is None:
            raise ValueError('delay_comp="queue" predicts under the commands in the line: it needs a delayed plant '
                             "(GpuPlant(..., delay=ActuationDelay(...)))")
        self.delay_comp = delay_comp
        if scorer is not None and scorer.B != x0.shape[0]:
            raise ValueError(f"the scorer holds {scorer.B} kites, the loop flies {x0.shape[0]}")
        if ekf and wind_ekf:
            raise ValueError("ekf and wind_ekf are two estimators: choose one")
        if kin_ekf and (ekf or wind_ekf):
            raise ValueError("kin_ekf, ekf and wind_ekf are three estimators: choose one")
        if estimator_model not in ("creation", "controller"):
            raise ValueError('estimator_model is "creation" or "controller"')
        if estimator_model == "controller" and kin_ekf:
            raise ValueError('estimator_model="controller" chooses a model: the kinematic filter has none')
        if estimator_model == "controller" and not (ekf or wind_ekf):
            raise ValueError('estimator_model="controller" needs an estimator: ekf=True or wind_ekf=True')
        if adapt is not None and recorder is None:
            raise ValueError("adapt identifies from a flight log: give the loop a recorder")
        joint = isinstance(ident_wind, str) and ident_wind == "joint"
        if isinstance(ident_wind, str) and not joint:
            if ident_wind != "estimate":
                raise ValueError('ident_wind is None, a (B, 3) tensor, "estimate" or "joint"')
            if not wind_ekf:
                raise ValueError('ident_wind="estimate" logs the wind EKF\'s estimate: it needs wind_ekf=True')
        if joint and adapt is None:
            raise ValueError('ident_wind="joint" identifies the wind with the 21: it needs adapt (and a recorder)')
        if ident_wind is not None and not joint and (recorder is None or getattr(recorder, "W", None) is None):
            raise ValueError("ident_wind is logged by the recorder: give the loop a FlightRecorder(..., wind=True)")
        B = x0.shape[0]
        dev = x0.device
        f64 = dict(dtype=torch.float64, device=dev)
        self.stepper, self.N, self.dt, self.pub, self.noise = stepper, N, dt, publisher, noise
        self.x0 = x0.clone()
        self.x_init = x0.clone()
        self.u0 = torch.zeros((B, 4), **f64)
        self.traj = torch.zeros((B, N + 1, 15), **f64)
        self.diag = torch.zeros((B, 6), **f64)
        self.status = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.ekf = ekf
        self.ekf_substeps = ekf_substeps
        if ekf:
            if covariances is None:
                raise ValueError("the EKF needs (W, V, P0)")
            W, V, P0 = (np.asarray(a, dtype=np.float64) for a in covariances)
            self.W = torch.from_numpy(W.copy()).to(dev)
            self.V = torch.from_numpy(V.copy()).to(dev)
            self.P = torch.from_numpy(np.repeat(P0[None], B, axis=0)).to(dev)
            self.P_init = self.P.clone()
            self.xe = self.x0[:, :13].clone()
            self.u3 = torch.zeros((B, 3), **f64)
            self.z = self.x0[:, 6:13].clone()
        # the wind-estimating EKF: xe = [x13 | W3] (the wind estimate starts at
        # 0), P 16 x 16; one fused call per step, then the estimated wind goes
        # to the controller's model on the device
        self.wind_ekf = wind_ekf
        self.wind_max = float(wind_max)
        if wind_ekf:
            if covariances is None:
                raise ValueError("the wind EKF needs (W, V, P0) in the 16-state shapes")
            W, V, P0 = (np.asarray(a, dtype=np.float64) for a in covariances)
            if W.shape != (16, 16) or V.shape != (7, 7) or P0.shape != (16, 16):
                raise ValueError("the wind EKF needs W (16, 16), V (7, 7), P0 (16, 16)")
            self.W = torch.from_numpy(W.copy()).to(dev)
            self.V = torch.from_numpy(V.copy()).to(dev)
            self.P = torch.from_numpy(np.repeat(P0[None], B, axis=0)).to(dev)
            self.P_init = self.P.clone()
            self.xe = torch.zeros((B, 16), **f64)
            self.xe[:, :13].copy_(self.x0[:, :13])
            self.u3 = torch.zeros((B, 3), **f64)
            self.z = self.x0[:, 6:13].clone()
            self.ekf_status = torch.zeros((B,), dtype=torch.int32, device=dev)
            self.wind_ekf_fresh = True
        # the kinematic EKF: xe = x13, P 13 x 13 with KiteEKF's covariances; one
        # fused call per step, no control and no model
        self.kin_ekf = kin_ekf
        if kin_ekf:
            if covariances is None:
                raise ValueError("the kinematic EKF needs (W, V, P0)")
            W, V, P0 = (np.asarray(a, dtype=np.float64) for a in covariances)
            if W.shape != (13, 13) or V.shape != (7, 7) or P0.shape != (13, 13):
                raise ValueError("the kinematic EKF needs W (13, 13), V (7, 7), P0 (13, 13)")
            self.W = torch.from_numpy(W.copy()).to(dev)
            self.V = torch.from_numpy(V.copy()).to(dev)
            self.P = torch.from_numpy(np.repeat(P0[None], B, axis=0)).to(dev)
            self.P_init = self.P.clone()
            self.xe = self.x0[:, :13].clone().contiguous()
            self.z = self.x0[:, 6:13].clone()
            self.ekf_status = torch.zeros((B,), dtype=torch.int32, device=dev)
            self.kin_ekf_fresh = True
        # the estimator filters with the controller's models in force (per kite
        # once ``adapt`` or set_params_device has set them) instead of the
        # creation model; "creation" calls nothing
        self.estimator_model = estimator_model
        if estimator_model == "controller":
            from . import nmpc
            stepper.set_estimator_model(nmpc.EST_MODEL_CONTROLLER)
        self.gathered = None
        # a ``FlightRecorder``: the state handed to the controller and the control
        # applied, one period per step, until it is full
        self.recorder = recorder
        # adapt (an ``IdentConfig``): each time the recorder is full the kites'
        # 21 aerodynamic coefficients are identified from it and become the
        # controller's per-kite models, all on the stream (``_adapt``)
        self.adapt = adapt
        self.adapt_count = 0
        # the wind the identification's model sees, logged each period next to the
        # control: None (no wind log), a known (B, 3) wind, or "estimate": the
        # wind in force for the controller this period, which is the wind EKF's
        # estimate as kite_nmpc_set_wind_device treats it (a non-finite
        # component 0, each clamped to +-wind_max)
        # "joint": no wind is known; ``adapt`` identifies a constant wind with the 21
        self.ident_wind = ident_wind
        self.ident_joint = joint
        if ident_wind is not None and not isinstance(ident_wind, str):
            if tuple(ident_wind.shape) != (B, 3):
                raise ValueError(f"ident_wind: a (B, 3) = ({B}, 3) tensor, got {tuple(ident_wind.shape)}")
            self.ident_wind = ident_wind.to(**f64).clone()
        if adapt is not None:
            from . import nmpc
            if recorder.B != B:
                raise ValueError(f"the recorder logs {recorder.B} kites, the loop flies {B}")
            i32 = dict(dtype=torch.int32, device=dev)
            self.model_rows = torch.from_numpy(np.ascontiguousarray(stepper.get_params(), dtype=np.float64)).to(dev)
            self.ident_rows = torch.zeros((B, 52), **f64)      # the last identification's result
            self.ident_cost2 = torch.zeros((B, 2), **f64)
            self.ident_evals = torch.zeros((B,), **i32)
            self.ident_status = torch.zeros((B,), **i32)       # KITE_IDENT_* of the last identification
            self.params_status = torch.zeros((B,), **i32)      # KITE_PARAMS_* of the last set_params_device
            # "joint": the wind is identified with the 21 (a constant offset per kite
            # on top of the recorder's wind log, zeros without one); no wind EKF and
            # no wind log is needed.  ident_wind_est holds the last identified offset
            if joint:
                self.ident_wind_config = (ident_wind_config if ident_wind_config is not None
                                          else nmpc.ident_wind_default_config())
                self.ident_wind_est = torch.zeros((B, 3), **f64)
                self._ident_wind_out = torch.zeros((B, 3), **f64)
                self._ident_ws = torch.empty((nmpc.ident_joint_workspace_doubles(adapt, B, recorder.T),), **f64)
            else:
                self._ident_ws = torch.empty((nmpc.ident_workspace_doubles(adapt, B, recorder.T),), **f64)
            self._ident_ok = nmpc.IDENT_CONVERGED, nmpc.IDENT_NAN
        # a plant of its own (``GpuPlant``, or any object with h, steps and
        # advance): the loop carries the true kite state xp and the time t
        self.plant = plant
        if plant is not None:
            if not math.isclose(plant.steps * plant.h, dt, rel_tol=1e-12, abs_tol=0.0):
                raise ValueError(f"plant: steps * h = {plant.steps * plant.h} is not the control period dt = {dt}")
            self.xp = x0[:, :13].clone().contiguous()
            self.t = 0.0
            self.plant_status = torch.zeros((B,), dtype=torch.int32, device=dev)
        # a delayed plant (``GpuPlant(..., delay=ActuationDelay)``): what flies is the
        # line's control in force, not u0.  The estimators propagate under it.  A
        # flight log holds one control per period, so it is kept only where the
        # control is constant over each period: no jitter, a whole number of periods
        self.delay = getattr(plant, "delay", None) if plant is not None else None
        if self.delay is not None:
            if self.delay.B != B:
                raise ValueError(f"the delay holds {self.delay.B} lines, the loop flies {B} kites")
            k = self.delay.mean / dt
            if recorder is not None and (self.delay.deviation != 0.0 or abs(k - round(k)) > 1e-9 * max(1.0, k)):
                raise ValueError("a recorder logs one control per period: with a delayed plant that is what flew "
                                 "only when deviation == 0 and mean is a whole number of control periods "
                                 f"(mean = {self.delay.mean}, deviation = {self.delay.deviation}, dt = {dt})")
        # a scorer (``EpisodeScore``): every period is scored right after the RTI,
        # one launch on the stream, from the true state at t0 and the control
        # just computed; None: no call is made
        self.scorer = scorer
        if scorer is not None:
            scorer.stepper, scorer.dt = stepper, dt
            if plant is None:
                self._score_x = torch.zeros((B, 13), **f64)

    def restart(self):
        """Start the next episode: every kite back at its launch state, the
        controller's next step a cold one (stepper.reset), the estimator at
        its initial estimate and covariance.  All on the stream, no sync."""
        self.stepper.reset()
        self.x0.copy_(self.x_init)
        self.u0.zero_()
        if self.scorer is not None:
            self.scorer.first = True   # the accumulators go on; the next period has no predecessor
        if self.adapt is not None:
            self.recorder.reset()      # a log does not span episodes; the adapted models (and wind) stay
        if self.plant is not None:
            self.xp.copy_(self.x_init[:, :13])
            self.t = 0.0
            self.plant_status.zero_()
        if self.delay is not None:
            self.delay.reset()
        if self.ekf:
            self.xe.copy_(self.x_init[:, :13])
            self.P.copy_(self.P_init)
            self.z.copy_(self.x_init[:, 6:13])
        if self.wind_ekf:
            self.xe.zero_()
            self.xe[:, :13].copy_(self.x_init[:, :13])
            self.P.copy_(self.P_init)
            self.z.copy_(self.x_init[:, 6:13])
            self.ekf_status.zero_()
            self.wind_ekf_fresh = True
        if self.kin_ekf:
            self.xe.copy_(self.x_init[:, :13])
            self.P.copy_(self.P_init)
            self.z.copy_(self.x_init[:, 6:13])
            self.ekf_status.zero_()
            self.kin_ekf_fresh = True

    def _adapt(self):
        """The full log becomes the controller's models, on the stream with no
        synchronisation: identify from the loop's current rows; a kite whose fit
        converged to a finite point takes the identified row, any other keeps
        its row; the rows go to the controller (a row that is no model is
        rejected there, ``params_status``); the log starts again with the state
        at hand.  This step's RTI already predicts with the new models."""
        rec = self.recorder
        if self.ident_joint:
            self.stepper.identify_joint(self.adapt, self.ident_wind_config, rec.T, self.model_rows, rec.X, rec.U,
                                        self.ident_rows, self._ident_wind_out, self.ident_cost2, self.ident_evals,
                                        self.ident_status, self._ident_ws, W0=getattr(rec, "W", None))
        elif getattr(rec, "W", None) is not None:
            self.stepper.identify(self.adapt, rec.T, self.model_rows, rec.X, rec.U, self.ident_rows, self.ident_cost2,
                                  self.ident_evals, self.ident_status, self._ident_ws, W=rec.W)
        else:
            self.stepper.identify(self.adapt, rec.T, self.model_rows, rec.X, rec.U, self.ident_rows,
                                  self.ident_cost2, self.ident_evals, self.ident_status, self._ident_ws)
        conv, nan = self._ident_ok
        ok = ((self.ident_status & conv) != 0) & ((self.ident_status & nan) == 0)
        self.model_rows.copy_(torch.where(ok[:, None], self.ident_rows, self.model_rows))
        self.stepper.set_params_device(self.model_rows, self.params_status)
        if self.ident_joint:
            # a kite whose fit did not converge keeps the wind it had; without a wind
            # EKF nobody else tells the controller the wind
            self.ident_wind_est.copy_(torch.where(ok[:, None], self._ident_wind_out, self.ident_wind_est))
            if not self.wind_ekf:
                self.ident_wind_est.clamp_(-self.wind_max, self.wind_max)
                self.stepper.set_wind_device(self.ident_wind_est, self.wind_max)
        self.adapt_count += 1
        rec.reset()
        rec.record_state(self.x0)

    def step(self):
        if self.wind_ekf:
            # the same propagation and update in one launch; the wind it
            # estimates is what the RTI's predictions assume from this step
            # on.  The first step of an episode has nothing to filter: xe is the
            # state measured at this instant, no time has passed under any
            # control.  (A propagation over dt followed by that stale
            # measurement is a position innovation of dt * v, which a filter
            # with a wind state books as several m/s of wind.)
            if self.wind_ekf_fresh:
                self.wind_ekf_fresh = False
            else:
                self.u3.copy_((self.u0 if self.delay is None else self.delay.u_applied)[:, :3])
                self.stepper.wind_ekf(self.dt, self.ekf_substeps, self.xe, self.u3, self.P, self.z, self.W, self.V,
                                      self.ekf_status)
            self.stepper.set_wind_device(self.xe[:, 13:], self.wind_max)
            self.x0[:, :13].copy_(self.xe[:, :13])
        if self.kin_ekf:
            # one launch: ekf_substeps propagations and the update.  The first
            # step of an episode filters nothing, as with the wind EKF: xe is
            # the state measured at this instant and no time has passed.
            if self.kin_ekf_fresh:
                self.kin_ekf_fresh = False
            else:
                self.stepper.kin_ekf(self.dt, self.ekf_substeps, self.xe, self.P, self.z, self.W, self.V,
                                     self.ekf_status)
            self.x0[:, :13].copy_(self.xe)
        if self.ekf:
            # propagate under the control applied last (u(t0) of the previous
            # plan; behind a delayed plant the line's control in force), update
            # with the measurement on the last substep
            self.u3.copy_((self.u0 if self.delay is None else self.delay.u_applied)[:, :3])
            h = self.dt / self.ekf_substeps
            for j in range(self.ekf_substeps):
                self.stepper.ekf(h, self.xe, self.u3, self.P, self.z if j == self.ekf_substeps - 1 else None,
                                 self.W, self.V)
            self.x0[:, :13].copy_(self.xe)
        if self.recorder is not None:
            self.recorder.record_state(self.x0)
            if self.adapt is not None and self.recorder.full:
                self._adapt()
        if self.delay_comp == "queue":
            # the lines as they stand now, at the instant the state was measured:
            # this step's delay compensation predicts under what is in flight
            self.stepper.set_inflight_device(self.delay.line, self.t)
        self.stepper.rti(self.x0, self.u0, self.traj, self.diag, self.status)
        if self.scorer is not None:
            # the true state at t0: the plant's, or without one the state the plan
            # started from (the loop's plant is then the plan itself)
            sc = self.scorer
            if self.plant is not None:
                self.stepper.score(self.xp, self.u0, self.status, self.plant_status, sc.first, sc.acc, sc.mem)
            else:
                self._score_x.copy_(self.x0[:, :13])
                self.stepper.score(self._score_x, self.u0, self.status, None, sc.first, sc.acc, sc.mem)
            sc.first = False
        if self.recorder is not None:
            if self.ident_joint:
                # the known part W0 of the joint model's wind: the wind EKF's estimate
                # where the loop runs one and the recorder logs a wind, else untouched
                if self.wind_ekf and getattr(self.recorder, "W", None) is not None:
                    w = torch.nan_to_num(self.xe[:, 13:16], nan=0.0, posinf=0.0, neginf=0.0)
                    self.recorder.record_wind(w.clamp(-self.wind_max, self.wind_max))
            elif self.ident_wind is not None:
                if isinstance(self.ident_wind, str):
                    w = torch.nan_to_num(self.xe[:, 13:16], nan=0.0, posinf=0.0, neginf=0.0)
                    self.recorder.record_wind(w.clamp(-self.wind_max, self.wind_max))
                else:
                    self.recorder.record_wind(self.ident_wind)
            if self.delay is None:
                self.recorder.record_control(self.u0)
        if self.pub is not None:
            self.gathered = self.pub.publish(self.u0, self.diag)
        if self.plant is None:
            self.x0.copy_(self.traj[:, 1, :])
        else:
            # the kite flies on under u(t0); it is measured at t0 + dt, theta and
            # thetadot come from the plan (nmpf_node.cpp:220)
            self.plant.advance(self.xp, self.u0, self.t, self.plant_status)
            if self.delay is not None and self.recorder is not None:
                self.recorder.record_control(self.delay.u_applied)    # what flew this period
            self.t += self.dt
            self.x0[:, :13].copy_(self.xp)
            self.x0[:, 13:].copy_(self.traj[:, 1, 13:])
        if self.noise is not None:
            self.noise.apply(self.x0)
        if self.ekf or self.wind_ekf or self.kin_ekf:
            self.z.copy_(self.x0[:, 6:13])
