"""What each solver of cd360.job.Sampler knows and the others do not: its per-schedule tables and buffers (`tables`), the rows the un-staged
route copies per step (`rows`), the tail kernel that ends a staged step, its un-staged step, and whether it draws noise.  One stateless
object per solver; the state lives on the Sampler `smp` they are handed, under the names tests and tools read, next to the buffers every
solver shares (smp.gx, smp.gi, smp._iota, smp.step_tab).  SOLVERS holds the one-evaluation solvers on the step table, EDM_SOLVERS the EDM
family (include/cd360_edm.h), HIGHORDER_SOLVERS DPM++ 2S ancestral and linear multistep (include/cd360_highorder.h); select() picks, by
the name, the churn and whether the schedule lies on the denoiser's grid."""
from __future__ import annotations

import torch

from . import ops
from . import sampler as S


GI = ("gi", "_iota")  # an entry of `rows`: the un-staged step reads the step index smp.gi as well (the sampler owns it; its values lie in _iota)


class Solver:
    """What the job asks of every solver; the defaults are those of a solver with one network evaluation per step, no table of its own and
    no noise."""

    draws_noise = False
    rows = ()  # (row buffer, table) names: smp.<buffer> holds the row of smp.<table> that the un-staged step reads; subclasses extend it
    single_last = False  # True: the sigma_next = 0 step differs in SHAPE from the others (fewer evaluations) and is captured on its own

    def single_row(self, smp, i) -> bool:
        """Does step i take ONE network evaluation where the solver's other steps take two?  Such rows run on a graph of their own
        (smp.lgraph) with smp.last_row set.  The default is Heun's answer: the last row only, for a solver that says single_last."""
        return self.single_last and i == smp.n_steps - 1

    def draws(self, smp) -> bool:
        return self.draws_noise

    def tables(self, smp, x):
        """The solver's per-schedule tables and the buffers it carries, on x's device."""

    def rows_of(self, smp):
        """`rows` for this sampler's schedule."""
        return self.rows

    def build(self, smp, x):
        self.tables(smp, x)
        for buf, tab in self.rows_of(smp):
            if (buf, tab) != GI:
                setattr(smp, buf, getattr(smp, tab)[0].clone())

    def build_stage(self, smp):
        """Staged route only, after the sampler's own tables exist: further stage-in tables."""

    def set_row(self, smp, i):
        for buf, tab in self.rows_of(smp):  # in the order declared
            getattr(smp, buf).copy_(getattr(smp, tab)[i:i + 1] if (buf, tab) == GI else getattr(smp, tab)[i])

    def staged_step(self, smp, evaluate):
        """One staged step in place on smp.gx.  `evaluate(x, tab, temb)` = stage-in on x with the step's row of `tab` / `temb` -> UNet trunk
        -> the output convolution's rows."""
        return self.tail(smp, evaluate(smp.gx, smp.step_tab, smp.temb_tab))

    @staticmethod
    def noise_buffers(smp, x):
        """The generator's seed / stream-id buffers the kernels read on the device (smp.noise_streams honoured), and the DeviceNoise on them."""
        smp.seed_buf = torch.tensor([S.seed_words(smp.seed)], dtype=torch.int64, device=x.device)
        smp.streams_buf = torch.zeros(x.shape[0], dtype=torch.int32, device=x.device)
        if smp.noise_streams is not None:
            smp.set_noise_streams(smp.noise_streams)
        smp.noise = S.DeviceNoise(smp.seed_buf, smp.streams_buf, smp.gi)

    @staticmethod
    def device_c_in(smp, *tabs):
        """c_in of each table's snapped sigma (column 3) through the denoiser's own module ON the device, as step_tab holds it and the
        module route computes it (the host's may differ in the last bit)."""
        for tab in tabs:
            tab[:, 2] = smp.denoiser.scaling(tab[:, 3])[2]


class Euler(Solver):
    """EulerEDMSampler (sampling.py:85-136) with s_churn = 0: sigma and sigma_next are all a step needs."""

    def tail(self, smp, eps_cl):  # [c_out, CFG, to_d, Euler]
        return ops.cfg_euler_step_cl(smp.gx, eps_cl, smp.step_tab, smp.gi, smp.scale, smp.scale_im)

    def step(self, smp, unet, x, s, s_next):
        return S.fused_cfg_euler_step(smp.denoiser, unet, x, s, s_next, smp.guider)


class DPMPP2M(Solver):
    """DPMPP2MSampler (sampling.py:390-465: second order, multistep, the same one UNet evaluation per step).  Off the denoiser's grid
    (smp.on_grid False) the tail's one scalar, c_out's, is the SNAPPED sigma: the staged tail takes smp.cout_tab in place of smp.step_tab,
    the un-staged one the row in smp.gq; the multipliers come from the schedule's own sigmas either way."""

    rows = (("gm", "mult_tab"),)
    off_grid_rows = rows + (("gq", "cout_tab"),)  # un-staged, off the grid: the step's row of cout_tab, whose element 0 is q(sigma_i)

    def rows_of(self, smp):
        return self.rows if smp.on_grid else self.off_grid_rows

    def tables(self, smp, x):
        """The multiplier table (host fp32, uploaded: the same bits in every sampler of a schedule) and gd = the previous step's denoised
        latent d0, shaped like gx and shared by both captured graphs.  retarget() does not reset gd: row 0 of the table has m4 = 0 and the
        kernels then never read it -- which is also why step(x, i) for i > 0 must follow step(., i - 1) of the same image."""
        smp.mult_tab = S.dpmpp2m_multipliers(smp.sigmas).to(x.device)
        smp.gd = torch.zeros_like(x)
        # cout_tab: step_tab with column 0 = q(sigma_i) -- on the grid step_tab ITSELF.  The staged sampler built step_tab before its
        # solver's tables; the un-staged route has none and reads cout_tab off the grid alone (rows_of)
        step_tab = getattr(smp, "step_tab", None)
        if step_tab is None and not smp.on_grid:
            step_tab = smp.step_table()[0]
        smp.cout_tab = None if step_tab is None else S.dpmpp2m_cout_table(step_tab, smp.sigmas, smp.denoiser, smp.on_grid)

    def tail(self, smp, eps_cl):  # x and gd in place: [c_out at q(sigma), CFG, multistep update]
        return ops.cfg_dpmpp2m_step_cl(smp.gx, smp.gd, eps_cl, smp.cout_tab, smp.mult_tab, smp.gi, smp.scale, smp.scale_im)

    def step(self, smp, unet, x, s, s_next):  # the kernel on the row in gm (off the grid: c_out's sigma in gq); this step's d0 moves into gd
        out, d0 = S.fused_cfg_dpmpp2m_step(smp.denoiser, unet, x, smp.gd, s, smp.gm, smp.guider, sigma_q=None if smp.on_grid else smp.gq[:1])
        smp.gd.copy_(d0)
        return out


class EulerAncestral(Solver):
    """EulerAncestralSampler (sampling.py:236-273, 340-347: stochastic; smp.eta / smp.s_noise as the reference's constructor takes them)."""

    draws_noise = True
    rows = (("ga", "anc_tab"), GI)  # (gi: the noise counter's step word on the un-staged route as well)

    def tables(self, smp, x):
        """The (sigma_down, sigma_up, s_noise, 0) table (host fp32, uploaded: the same bits in every sampler of a schedule) and the
        generator's seed / stream-id buffers the tail kernels read on the device.  Nothing is carried from one step to the next."""
        smp.anc_tab = S.euler_ancestral_table(smp.sigmas, smp.eta, smp.s_noise).to(x.device)
        self.noise_buffers(smp, x)

    def tail(self, smp, eps_cl):  # [c_out, CFG, to_d, Euler to sigma_down, + noise sigma_up]
        return ops.cfg_euler_ancestral_step_cl(smp.gx, eps_cl, smp.step_tab, smp.anc_tab, smp.gi, smp.seed_buf, smp.streams_buf, smp.scale,
                                               smp.scale_im)

    def step(self, smp, unet, x, s, s_next):  # the kernel on the row in ga and the step index in gi
        return S.fused_cfg_euler_ancestral_step(smp.denoiser, unet, x, s, smp.ga, smp.guider, noise=smp.noise)


SOLVERS = {"euler": Euler(), "dpmpp2m": DPMPP2M(), "euler_a": EulerAncestral()}


class ChurnedEuler(Solver):
    """EulerEDMSampler with s_churn > 0 (sampling.py:96-136): noise in front of the network on the rows of the s_tmin / s_tmax window, the
    network at q(sigma_hat), the Euler step from the un-snapped sigma_hat (include/cd360_edm.h).  smp.s_churn / s_tmin / s_tmax / s_noise as
    the reference's constructor takes them."""

    rows = (("ge", "edm_tab"), ("gc", "corr_tab"), GI)  # (gi: the churn table's row and the noise counter's step word on the un-staged route)

    def draws(self, smp) -> bool:
        return smp.s_churn > 0

    def tables(self, smp, x):
        """The three tables of cd360.sampler.edm_tables (host fp32, uploaded: the same bits in every sampler of a schedule; c_in re-derived
        on the device from the uploaded snapped sigma, so an un-churned row is step_tab's row bit for bit) and, where the schedule churns,
        the generator's buffers the churn kernel reads on the device.  Nothing is carried from one step to the next."""
        smp.edm_tab, smp.corr_tab, smp.churn_tab = (t.to(x.device) for t in S.edm_tables(smp.sigmas, smp.denoiser, smp.s_churn, smp.s_tmin,
                                                                                           smp.s_tmax, smp.s_noise))
        self.device_c_in(smp, smp.edm_tab, smp.corr_tab)
        smp.churned = bool((smp.churn_tab[:, 1] > 0).any())  # (once per schedule; a step reads nothing back)
        smp.noise = None
        if self.draws(smp):
            self.noise_buffers(smp, x)

    def build_stage(self, smp):  # the time-embedding rows of q(sigma_hat): the network is evaluated there, not at sigma_i
        smp.edm_temb = smp.temb_rows(smp.edm_tab[:, 3])

    def predict(self, smp, evaluate, xe, d=None):  # [churn] -> stage-in on edm_tab -> trunk -> [c_out at q(sigma_hat), CFG, to_d, Euler]
        if smp.churned:  # its own launch in front of stage-in, which reads a 3x3 halo of gx
            ops.edm_churn(smp.gx, smp.churn_tab, smp.gi, smp.seed_buf, smp.streams_buf)
        eps_cl = evaluate(smp.gx, smp.edm_tab, smp.edm_temb)
        return ops.cfg_edm_predict_cl(smp.gx, eps_cl, smp.edm_tab, smp.gi, smp.scale, smp.scale_im, xe, d)

    def staged_step(self, smp, evaluate):  # in place
        return self.predict(smp, evaluate, smp.gx)

    def step(self, smp, unet, x, s, s_next):  # the kernels on the rows in ge / gc and the step index in gi
        return S.fused_cfg_edm_euler_step(smp.denoiser, unet, x, smp.ge, smp.churn_tab if smp.churned else None, smp.guider, noise=smp.noise)


class Heun(ChurnedEuler):
    """HeunEDMSampler (sampling.py:321-337: second order, TWO network evaluations per step, one on the sigma_next = 0 step; churn as for
    Euler).  smp.gxe = the predictor's x_e and smp.gdir = its direction d, shaped like gx: both are written before they are read within a
    step, so retarget() resets neither.  smp.last_row (set by the sampler: on the last step, and while it captures that step's graph)
    is the reference's host-side skip of the corrector."""

    single_last = True

    def tables(self, smp, x):
        super().tables(smp, x)
        smp.gxe, smp.gdir = torch.zeros_like(x), torch.zeros_like(x)

    def build_stage(self, smp):  # the corrector's evaluation: the network at q(sigma_next)
        super().build_stage(smp)
        smp.corr_temb = smp.temb_rows(smp.corr_tab[:, 3])

    def staged_step(self, smp, evaluate):
        if smp.last_row:
            return super().staged_step(smp, evaluate)
        self.predict(smp, evaluate, smp.gxe, smp.gdir)
        eps2_cl = evaluate(smp.gxe, smp.corr_tab, smp.corr_temb)  # h0 and emb_act are reused
        return ops.cfg_edm_correct_cl(smp.gx, smp.gxe, smp.gdir, eps2_cl, smp.edm_tab, smp.corr_tab, smp.gi, smp.scale, smp.scale_im)

    def step(self, smp, unet, x, s, s_next):
        return S.fused_cfg_heun_step(smp.denoiser, unet, x, smp.ge, smp.gc, smp.churn_tab if smp.churned else None, smp.guider, noise=smp.noise,
                                     last=smp.last_row)


# the EDM family on include/cd360_edm.h: "heun", and the object solver="euler" runs on when s_churn > 0 (select(), below)
EDM_SOLVERS = {"euler": ChurnedEuler(), "heun": Heun()}


class DPMPP2SAncestral(EulerAncestral):
    """DPMPP2SAncestralSampler (sampling.py:350-387: second order, single step, TWO network evaluations per step -- the second at the
    midpoint sigma_mid, off the denoiser's grid -- and the ancestral noise of EulerAncestralSampler; smp.eta / smp.s_noise as the reference's
    constructor takes them).  A row with sigma_down = 0 (the last; for eta > 1 interior rows as well: smp.single_rows) takes one evaluation
    and is exactly the ancestral Euler step: it runs the parent's tail, on the one-evaluation graph.  smp.gx2 = the midpoint latent,
    written before it is read within a step, so retarget() does not reset it."""

    rows = EulerAncestral.rows + (("gmid", "mid_tab"), ("gm2s", "mult2s_tab"))

    def tables(self, smp, x):
        """EulerAncestral's table and generator buffers, then the two further tables of cd360.sampler.dpmpp2s_tables (host fp32, uploaded;
        c_in of the second evaluation re-derived on the device), the host list of the one-evaluation rows, and gx2."""
        super().tables(smp, x)
        anc, mid, mult = S.dpmpp2s_tables(smp.sigmas, smp.denoiser, smp.eta, smp.s_noise)  # (anc: the table super().tables uploaded)
        smp.single_rows = S.dpmpp2s_single_rows(anc)
        smp.mid_tab, smp.mult2s_tab = mid.to(x.device), mult.to(x.device)
        self.device_c_in(smp, smp.mid_tab)
        smp.gx2 = torch.zeros_like(x)

    def single_row(self, smp, i) -> bool:
        return smp.single_rows[i]

    def build_stage(self, smp):  # the second evaluation: the network at q(sigma_mid)
        smp.mid_temb = smp.temb_rows(smp.mid_tab[:, 3])

    def staged_step(self, smp, evaluate):
        if smp.last_row:  # one evaluation -> the ancestral Euler tail
            return super().staged_step(smp, evaluate)
        eps_cl = evaluate(smp.gx, smp.step_tab, smp.temb_tab)
        ops.cfg_dpmpp2s_mid_cl(smp.gx, eps_cl, smp.step_tab, smp.mult2s_tab, smp.gi, smp.scale, smp.scale_im, smp.gx2)
        eps2_cl = evaluate(smp.gx2, smp.mid_tab, smp.mid_temb)  # h0 and emb_act are reused
        return ops.cfg_dpmpp2s_step_cl(smp.gx, smp.gx2, eps2_cl, smp.mid_tab, smp.mult2s_tab, smp.anc_tab, smp.gi, smp.seed_buf, smp.streams_buf,
                                       smp.scale, smp.scale_im)

    def step(self, smp, unet, x, s, s_next):  # the kernels on the rows in ga / gmid / gm2s and the step index in gi
        return S.fused_cfg_dpmpp2s_step(smp.denoiser, unet, x, s, smp.ga, smp.gmid, smp.gm2s, smp.guider, noise=smp.noise, single=smp.last_row)


class LMS(Solver):
    """LinearMultistepSampler (sampling.py:276-311: Adams-Bashforth of order smp.order <= 4 over the sigma schedule, one UNet evaluation per
    step, deterministic)."""

    rows = (("gl", "lms_tab"), GI)  # (gi names the ring slot on the un-staged route as well)

    def tables(self, smp, x):
        """The coefficient table (host, uploaded: the same bits in every sampler of a schedule) and gds = the ring of the last `order`
        directions, [order, *x.shape], shared by both captured graphs.  retarget() does not reset it: step i reads only the min(i + 1,
        order) - 1 slots written by the steps before it, so row 0 reads no old slot -- which is also why step(x, i) for i > 0 must follow
        step(., i - 1) of the same image."""
        smp.lms_tab = S.lms_coefficients(smp.sigmas, smp.order).to(x.device)
        smp.gds = torch.zeros((smp.order,) + tuple(x.shape), dtype=x.dtype, device=x.device)

    def tail(self, smp, eps_cl):  # x and the ring in place: [c_out, CFG, to_d, multistep sum]
        return ops.cfg_lms_step_cl(smp.gx, smp.gds, eps_cl, smp.step_tab, smp.lms_tab, smp.gi, smp.scale, smp.scale_im)

    def step(self, smp, unet, x, s, s_next):  # the kernel on the row in gl and the step index in gi
        return S.fused_cfg_lms_step(smp.denoiser, unet, x, smp.gds, s, smp.gl, smp.gi, smp.guider)


# the solvers on include/cd360_highorder.h
HIGHORDER_SOLVERS = {"dpmpp2s_a": DPMPP2SAncestral(), "lms": LMS()}
NAMES = tuple(SOLVERS) + tuple(k for k in EDM_SOLVERS if k not in SOLVERS) + tuple(HIGHORDER_SOLVERS)  # every solver name, once


OFF_GRID = ("euler", "heun", "dpmpp2m")  # the solvers whose kernels take the snapped sigma (c_out) and the schedule's own (to_d, dt) apart


def select(name, s_churn=0.0, on_grid=True) -> Solver:
    """The object that serves `name`.  A name two registries share ("euler") is the EDM family's as soon as the schedule churns or leaves
    the denoiser's grid (cd360.sampler.on_grid: its tables hold sigma_hat and the snapped sigma side by side; with gamma = 0 no churn
    kernel runs), and SOLVERS' own otherwise (kernels and launch count of the un-churned on-grid step unchanged).  The tails of the
    remaining solvers read ONE sigma for c_out and for to_d: off the grid they are refused."""
    if not on_grid and name not in OFF_GRID:
        raise ValueError(f"solver {name!r} reads one sigma per step for c_out and to_d, and this schedule does not lie on the denoiser's grid "
                         f"(a Karras or listed schedule): off the grid the job sampler serves {', '.join(OFF_GRID)}")
    edm = name in EDM_SOLVERS and (name not in SOLVERS or s_churn > 0 or not on_grid)
    return (EDM_SOLVERS if edm else HIGHORDER_SOLVERS if name in HIGHORDER_SOLVERS else SOLVERS)[name]
