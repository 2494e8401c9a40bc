"""KL (Karhunen-Loeve) screens on the MI355X (kl_screen.py:22-449 of the
reference).

``KLScreen`` keeps the reference's constructor and methods.  ``fit`` runs the
batched GPU fit (``stationscreen.run`` -> ``sf_kl_fit``: the fit-pass,
subset-eigenbasis and classify kernels of csrc/kl_fit_fast.hip);
``make_matrix`` and ``write`` evaluate the screens with ``sf_kl_eval`` (the
LDS-staged ``kl_eval_lds_kernel`` or the register-tile ``kl_eval_kernel`` of
csrc/kl_eval.hip, chosen per D: an MFMA float64 contraction + sincos
epilogue) instead of a per-pixel Python loop in a process pool.  ``sample``
and ``patch_errors`` evaluate them at sky positions only
(``sf_kl_eval_points``, csrc/kl_points.hip): what the cube holds at the
calibrator patches -- the reference's acceptance quantity -- without the cube.
"""

import multiprocessing

import numpy as np

from . import geometry
from . import stationscreen
from ._lib import (SF_EVAL_BIG_ENDIAN, SF_EVAL_FAST_SINCOS, SF_EVAL_NAN_SCRUB,
                   SF_EVAL_NT_STORES, SF_MAX_DIR, SF_MAX_POINTS, Context)
from .h5parm import H5parm, get_reference_station
from .screen import Screen, canonical_axes, phase_pols
from .streaming import batch_rows, stream_time_rows

# NaN scrub (screen.py:368-378) + exact fp64 reduction of the phase in
# revolutions / hardware fp32 sincos + streaming stores
DEFAULT_FLAGS = SF_EVAL_NAN_SCRUB | SF_EVAL_FAST_SINCOS | SF_EVAL_NT_STORES


def read_patch_names(skymodel_filename):
    """Patch names of a makesourcedb sky model (the patch lines ``, , name,
    ra, dec``), i.e. the keys of lsmtool ``getPatchPositions()``."""
    names = []
    with open(skymodel_filename, encoding="utf8") as fh:
        for line in fh:
            parts = [p.strip() for p in line.split(",")]
            if len(parts) >= 5 and parts[0] == "" and parts[1] == "" and parts[2]:
                names.append(parts[2])
    return names


def tec_channel_groups(tec_index, n_tec_freq):
    """The launches of ``sf_kl_eval_tec`` for the channel binding
    ``tec_index`` [F] over ``n_tec_freq`` TEC frequencies: a list of
    ``(i, channels)``, one entry per TEC frequency i that some channel refers
    to, in ascending i, ``channels`` the int array of its output channels in
    ascending order.  A frequency without channels has no entry: its
    coefficients are never read.  Raises ValueError for an index outside
    ``0..n_tec_freq-1`` (the C side's SF_EINVAL)."""
    idx = np.asarray(tec_index, np.int64).reshape(-1)
    if int(n_tec_freq) < 1:
        raise ValueError(f"n_tec_freq: {n_tec_freq}, expected >= 1")
    if idx.size and (idx.min() < 0 or idx.max() >= int(n_tec_freq)):
        raise ValueError(f"tec_index: values {idx.min()}..{idx.max()} outside "
                         f"0..{int(n_tec_freq) - 1}")
    order = np.argsort(idx, kind="stable")
    used, start = np.unique(idx[order], return_index=True)
    return [(int(i), order[a:b]) for i, a, b in
            zip(used, start, list(start[1:]) + [idx.size])]


class KLEvaluator:
    """Device state for evaluating KL screens on one grid and / or at a list
    of positions.  Owns its sf_ctx: the basis, pixel grid and points it sets
    stay put whatever other screens or the fit (which takes a
    ``private_context`` per call) set meanwhile."""

    def __init__(self, piercepoints, r_0, beta, x_coord=None, y_coord=None,
                 device=0):
        import torch

        self.torch = torch
        self.dev = torch.device("cuda", device)
        self.ctx = Context(device)
        self.pp = np.asarray(piercepoints, np.float64)
        self.D = self.pp.shape[0]
        if (x_coord is None) != (y_coord is None):
            raise ValueError("give both grid coordinates or neither")
        self.nx, self.ny = (0, 0) if x_coord is None else (len(x_coord), len(y_coord))
        self.n_points = 0
        with torch.cuda.device(self.dev):
            self.ctx.set_stream(torch.cuda.current_stream(self.dev).cuda_stream)
            if self.D > SF_MAX_DIR:
                # evaluation needs no eigen-basis: up to SF_MAX_EVAL_DIR
                self.ctx.set_piercepoints(self.pp, r_0, beta)
            else:
                self.ctx.set_basis(self.pp, r_0, beta)
            if x_coord is not None:
                self.ctx.set_grid(x_coord, y_coord)

    def _launch(self, call, out_dev=None, shape=None, dtype=None):
        """``call(out_dev)`` on this evaluator's device, its context bound to
        the current stream; ``out_dev`` is allocated unless given (``shape``,
        float32 unless ``dtype``) and returned."""
        torch = self.torch
        if out_dev is None and shape is not None:
            out_dev = torch.empty(shape, dtype=dtype or torch.float32, device=self.dev)
        with torch.cuda.device(self.dev):
            self.ctx.set_stream(torch.cuda.current_stream(self.dev).cuda_stream)
            call(out_dev)
        return out_dev

    def _host(self, coef, tail, run):
        """Host [..., D] coefficients in, host ``lead + tail`` out: ``run``
        takes the uploaded [S, D] coefficients and returns the device result."""
        lead = np.shape(coef)[:-1]
        return run(self._upload(coef)).cpu().numpy().reshape(lead + tail)

    def _upload(self, a, shape=None):
        """Host array as a float64 device tensor, [S, D] unless ``shape``."""
        a = np.ascontiguousarray(a, np.float64)
        return self.torch.from_numpy(a.reshape(shape or (-1, self.D))).to(self.dev)

    def _upload_opt(self, a):
        return None if a is None else self._upload(a)

    def set_points(self, xy):
        """Bind P screen positions ``xy`` [P, 2] (piercepoint coordinates,
        ``geometry.screen_xy``) for ``sample_device`` / ``sample_host``."""
        self._launch(lambda _: self.ctx.set_points(xy))
        self.n_points = self.ctx.points

    def sample_device(self, coef_dev, xx_dev=None, yy_dev=None, out_dev=None,
                      values=False, flags=SF_EVAL_NAN_SCRUB | SF_EVAL_FAST_SINCOS):
        """coef_dev: device [S, D] float64 -> device [S, 4, P] float32 Jones
        planes at the bound points (gain planes with ``xx_dev`` / ``yy_dev``),
        or, with ``values``, the screen values [S, P] float64."""
        S, P = coef_dev.shape[0], self.n_points
        if values:
            return self._launch(lambda out: self.ctx.eval_point_values(coef_dev, S, out),
                                out_dev, (S, P), self.torch.float64)
        return self._launch(
            lambda out: self.ctx.eval_points(coef_dev, S, out, xx_dev, yy_dev, flags),
            out_dev, (S, 4, P))

    def sample_host(self, coef, amp_xx=None, amp_yy=None, values=False,
                    flags=SF_EVAL_NAN_SCRUB | SF_EVAL_FAST_SINCOS):
        """Host [..., D] coefficients -> host float32 [..., 4, P] planes, or
        float64 [..., P] values."""
        if values:
            return self._host(coef, (self.n_points,),
                              lambda c: self.sample_device(c, values=True))
        return self._host(coef, (4, self.n_points), lambda c: self.sample_device(
            c, self._upload_opt(amp_xx), self._upload_opt(amp_yy), flags=flags))

    def eval_device(self, coef_dev, out_dev=None, flags=DEFAULT_FLAGS):
        """coef_dev: device [S, D] float64 -> device [S, 4, ny, nx] float32."""
        S = coef_dev.shape[0]
        return self._launch(lambda out: self.ctx.eval(coef_dev, S, out, S, flags),
                            out_dev, (S, 4, self.ny, self.nx))

    def eval_gain_device(self, coef_dev, xx_dev, yy_dev, out_dev=None,
                         flags=DEFAULT_FLAGS):
        """Phase + XX / YY log10-amplitude coefficients (device [S, D] each)
        -> device [S, 4, ny, nx] gain planes."""
        S = coef_dev.shape[0]
        return self._launch(
            lambda out: self.ctx.eval_gain(coef_dev, xx_dev, yy_dev, S, out, S, flags),
            out_dev, (S, 4, self.ny, self.nx))

    def eval_pol_device(self, xx_dev, yy_dev, out_dev=None, amp_xx_dev=None,
                        amp_yy_dev=None, flags=DEFAULT_FLAGS):
        """Polarized phases (``sf_kl_eval_pol``): the XX and YY phase
        coefficients (device [S, D] each), and optionally the XX and YY
        log10-amplitude coefficients (both or neither) -> device
        [S, 4, ny, nx]: planes 0 / 1 from XX, planes 2 / 3 from YY."""
        S = xx_dev.shape[0]
        return self._launch(
            lambda out: self.ctx.eval_pol(xx_dev, yy_dev, S, out, S, amp_xx_dev,
                                          amp_yy_dev, flags),
            out_dev, (S, 4, self.ny, self.nx))

    def eval_pol_host(self, coef_xx, coef_yy, amp_xx=None, amp_yy=None,
                      flags=DEFAULT_FLAGS):
        """XX / YY phase coefficients (and optional log10-amplitude coefs):
        host [..., D] -> host float32 [..., 4, ny, nx]."""
        return self._host(coef_xx, (4, self.ny, self.nx), lambda c: self.eval_pol_device(
            c, self._upload(coef_yy), amp_xx_dev=self._upload_opt(amp_xx),
            amp_yy_dev=self._upload_opt(amp_yy), flags=flags))

    def values_device(self, coef_dev, out_dev=None, flags=0):
        """coef_dev: device [S, D] float64 -> device [S, ny, nx] float32, the
        screen values themselves in the coefficients' units (``sf_kl_eval_values``:
        fp64 contraction, one cast; NaN where a coefficient is NaN unless
        ``flags`` scrub it to 0; plain stores: streaming stores measured no
        faster for this kernel)."""
        S = coef_dev.shape[0]
        return self._launch(lambda out: self.ctx.eval_values(coef_dev, S, out, S, flags),
                            out_dev, (S, self.ny, self.nx))

    def values_host(self, coef, flags=0):
        """Host [..., D] coefficients -> host float32 [..., ny, nx] values."""
        return self._host(coef, (self.ny, self.nx),
                          lambda c: self.values_device(c, flags=flags))

    def eval_tec_device(self, tec_dev, rad_per_tecu, tec_index=None, phase_dev=None,
                        out_dev=None, flags=DEFAULT_FLAGS):
        """TEC screens to Jones planes at F channels (``sf_kl_eval_tec``):
        ``tec_dev`` device [T, F_tec, A, D] float64 in TECU, ``rad_per_tecu``
        [F] (= tec_to_phase / nu), ``tec_index`` [F] the TEC frequency each
        channel takes (default: 0, for F_tec = 1), ``phase_dev`` None or the
        frequency-independent phase screens in radians, shaped as ``tec_dev``
        -> device [T, F, A, 4, ny, nx] float32 of the phase
        ``rad_per_tecu[f] * dTEC + phi0``.  One contraction per (time, TEC
        frequency, station); no coefficients are replicated per channel."""
        if tec_dev.dim() != 4 or tec_dev.shape[3] != self.D:
            raise ValueError(f"tec_dev: shape {tuple(tec_dev.shape)}, expected "
                             f"(T, F_tec, A, {self.D})")
        T, F_tec, A, _ = tec_dev.shape
        k = np.asarray(rad_per_tecu, np.float64).reshape(-1)
        if tec_index is None:
            if F_tec != 1:
                raise ValueError("tec_index: needed for more than one tec frequency")
        else:
            tec_channel_groups(tec_index, F_tec)  # range check
        if phase_dev is not None and phase_dev.shape != tec_dev.shape:
            raise ValueError(f"phase_dev: shape {tuple(phase_dev.shape)}, expected "
                             f"{tuple(tec_dev.shape)}")

        def call(out):
            self._bind_tec_freqs(k, tec_index, F_tec)
            self.ctx.eval_tec(tec_dev, T, A, out, phase_dev, flags)

        return self._launch(call, out_dev, (T, k.size, A, 4, self.ny, self.nx))

    def _bind_tec_freqs(self, k, tec_index, F_tec):
        """sf_set_tec_freqs unless this binding is the context's already (it
        synchronises: a write's batches share one binding)."""
        idx = None if tec_index is None else np.asarray(tec_index, np.int32).reshape(-1)
        key = (k.tobytes(), None if idx is None else idx.tobytes(), int(F_tec))
        if getattr(self, "_tec_key", None) != key:
            self._tec_key = None
            self.ctx.set_tec_freqs(k, idx, F_tec)
            self._tec_key = key

    def eval_tec_host(self, tec_coef, rad_per_tecu, tec_index=None, phase_coef=None,
                      flags=DEFAULT_FLAGS):
        """Host [T, F_tec, A, D] TEC (and optional phase) coefficients -> host
        float32 [T, F, A, 4, ny, nx] (``eval_tec_device``)."""
        out = self.eval_tec_device(
            self._upload(tec_coef, np.shape(tec_coef)), rad_per_tecu, tec_index,
            None if phase_coef is None else self._upload(phase_coef, np.shape(phase_coef)),
            flags=flags)
        return out.cpu().numpy()

    def smooth_device(self, out_dev, smooth_pix, flags):
        """Screen.write's Gaussian (screen.py:353-362) in place on a device
        cube [S, 4, ny, nx]; scrub / byte swap in ``flags`` after it."""
        return self._launch(
            lambda out: self.ctx.smooth(out, self.nx, self.ny, 4 * out.shape[0],
                                        smooth_pix, flags), out_dev)

    def eval_host(self, coef, amp_xx=None, amp_yy=None, flags=DEFAULT_FLAGS):
        """coef (and optional log10-amplitude coefs): host [..., D] -> host
        float32 [..., 4, ny, nx]."""
        if amp_xx is None:
            return self._host(coef, (4, self.ny, self.nx),
                              lambda c: self.eval_device(c, flags=flags))
        return self._host(coef, (4, self.ny, self.nx), lambda c: self.eval_gain_device(
            c, self._upload(amp_xx), self._upload(amp_yy), flags=flags))


class KLBase(Screen):
    """What the KL screen classes share: the geometry a fit leaves on the
    screen soltab, and the grid evaluator built from it."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.height = None
        self.beta_val = None
        self.r_0 = None
        self.piercepoints = None
        self.mid_ra = None
        self.mid_dec = None
        self.ref_ind = None
        self._evaluators = {}

    def _check_sky_model(self, dirs):
        """KeyError (as the reference raises, kl_screen.py:79) for directions
        the sky model, if there is one, has no patch for."""
        if self.input_skymodel_filename is not None:
            patches = set(read_patch_names(self.input_skymodel_filename))
            missing = [d for d in dirs if d.strip("[]") not in patches]
            if missing:
                raise KeyError(f"directions not in the sky model: {missing}")

    def _adopt_screen_soltab(self, st, solset):
        """The axes and attributes of the fitted screen soltab ``st``; its
        values (``vals_ph``) are the caller's to shape."""
        self.times_ph = np.asarray(st.time)
        self.freqs_ph = np.asarray(st.freq)
        self.source_names = st.dir
        self.source_dict = solset.get_source()
        self.source_positions = [self.source_dict[s] for s in self.source_names]
        self.station_names = st.ant
        self.station_dict = solset.get_ant()
        self.station_positions = [self.station_dict[s] for s in self.station_names]
        self.height = st.attrs["height"]
        self.beta_val = st.attrs["beta"]
        self.r_0 = st.attrs["r_0"]
        self.piercepoints = np.array(st.piercepoint)
        self.mid_ra = st.attrs["midra"]
        self.mid_dec = st.attrs["middec"]

    def _memory_usage(self, cellsize_deg, n_freq, planes):
        """GB per time slot of a [1, n_freq, A, planes, ny, nx] array, the
        reference's estimate (kl_screen.py:157-190: int() sizes, 8-byte
        values, /10 overhead, x ncpu) so that time chunking matches."""
        ncpu = self.ncpu or multiprocessing.cpu_count()
        ximsize = int(self.width_ra / cellsize_deg)
        yimsize = int(self.width_dec / cellsize_deg)
        nbytes = 8 * n_freq * len(self.station_names) * planes * yimsize * ximsize
        return nbytes / 1024 ** 3 / 10 * ncpu

    def evaluator(self, cellsize_deg):
        key = float(cellsize_deg)
        ev = self._evaluators.get(key)
        if ev is None:
            x, y = geometry.grid_coords(self.rad, self.dec, self.width_ra,
                                        cellsize_deg, self.mid_ra, self.mid_dec)
            ev = KLEvaluator(self.piercepoints, self.r_0, self.beta_val, x, y,
                             self.device)
            self._evaluators = {key: ev}
        return ev


class KLScreen(KLBase):
    """Class for KL (Karhunen-Lo`eve) screens (kl_screen.py:22)."""

    def __init__(self, name, h5parm_filename, skymodel_filename, rad, dec,
                 width_ra, width_dec, solset_name="sol000",
                 phase_soltab_name="phase000", amplitude_soltab_name=None):
        super().__init__(name, h5parm_filename, skymodel_filename, rad, dec,
                         width_ra, width_dec, solset_name=solset_name,
                         phase_soltab_name=phase_soltab_name,
                         amplitude_soltab_name=amplitude_soltab_name)
        self._sampler = None
        self.solset = None

    def fit(self):
        """Fit screens to the input solutions (kl_screen.py:61-155): phases
        with per-station orders referenced to a central station; for gain
        solutions also the XX / YY log10 amplitudes (order
        min(12, max(3, round(D / 2))), 3 iterations, no order scaling).  A
        phase soltab with a ``pol`` axis of length 2 (XX, YY: a diagonal-mode
        solve) is fitted per pol, as ``stationscreen.run`` does for any pol
        axis: ``vals_ph`` is then [time, freq, ant, dir, 2] and ``pol_phases``
        is set; length 1 is the scalar case, any other length a ValueError."""
        self._evaluators = {}  # a refit invalidates the evaluated basis
        self._sampler = None
        h5 = H5parm(self.input_h5parm_filename)
        solset = h5.get_solset(self.input_solset_name)
        soltab_ph = solset.get_soltab(self.input_phase_soltab_name)
        dirs = [str(d) for d in soltab_ph.dir]
        self.pol_phases = phase_pols(soltab_ph) == 2
        self._check_sky_model(dirs)
        ref_ind = get_reference_station(soltab_ph, 10)
        screen_order = min(20, len(dirs) - 1)
        stationscreen.run(soltab_ph, "phase_screen000", order=screen_order,
                          ref_ant=ref_ind, scale_order=True, adjust_order=True,
                          ncpu=self.ncpu or 0, device=self.device)
        if not self.phase_only:
            soltab_amp = solset.get_soltab(self.input_amplitude_soltab_name)
            order_amp = min(12, max(3, int(np.round(len(dirs) / 2))))
            stationscreen.run(soltab_amp, "amplitude_screen000", order=order_amp,
                              niter=3, scale_order=False, adjust_order=True,
                              ncpu=self.ncpu or 0, device=self.device)
            sta = solset.get_soltab("amplitude_screen000")
            self.log_amps = True
            self.vals_amp = sta.val
            self.times_amp = np.asarray(sta.time)
            self.freqs_amp = np.asarray(sta.freq)
        st = solset.get_soltab("phase_screen000")
        self.vals_ph = canonical_axes(st, st.val)
        self._adopt_screen_soltab(st, solset)
        # the input and screen soltabs (in memory) and the reference station,
        # for patch_errors
        self.solset = solset
        self.ref_ind = ref_ind
        h5.close()

    def get_memory_usage(self, cellsize_deg):
        """GB per time slot of the Jones cube (``_memory_usage``)."""
        return self._memory_usage(cellsize_deg, len(self.freqs_ph), 4)

    def make_matrix(self, t_start_index, t_stop_index, freq_ind, stat_ind,
                    cellsize_deg, out_dir, ncpu):
        """(t_stop - t_start, 4, ny, nx) float64 (kl_screen.py:192-380): the
        raw cos / sin (x 10 ** amplitude) planes, NaN where a coefficient is
        NaN -- the reference scrubs NaNs only in ``Screen.write``, after the
        optional smoothing (screen.py:353-378), and so does ``write_chunk``.
        The values carry the float32 rounding of the FITS cube (Q12)."""
        del out_dir, ncpu
        sl = np.s_[t_start_index:t_stop_index, freq_ind, stat_ind]
        coef = np.asarray(self.vals_ph)[sl]
        ev = self.evaluator(cellsize_deg)
        flags = DEFAULT_FLAGS & ~SF_EVAL_NAN_SCRUB
        amp = (None, None)
        if not self.phase_only:
            a = np.asarray(self.vals_amp)[sl]
            amp = (a[..., 0], a[..., 1])
        if self.pol_phases:
            # planes 0 / 1 from the XX phase screens, 2 / 3 from the YY ones
            return ev.eval_pol_host(coef[..., 0], coef[..., 1], amp[0], amp[1],
                                    flags=flags).astype(np.float64)
        return ev.eval_host(coef, amp[0], amp[1], flags=flags).astype(np.float64)

    def write_chunk(self, writer, g_start, g_stop, cellsize_deg, smooth_pix,
                    max_batch_bytes=1 << 30):
        """All (freq, station) screens of times [g_start, g_stop): device
        batches of whole time rows in FITS byte order, streamed through
        pinned buffers to the file while the next batch is evaluated."""
        ev = self.evaluator(cellsize_deg)
        vals = np.asarray(self.vals_ph)[g_start:g_stop]
        slots = vals.shape[1] * vals.shape[2]  # per time row
        if self.pol_phases:
            coef, coef_y = ev._upload(vals[..., 0]), ev._upload(vals[..., 1])
        else:
            coef = ev._upload(vals)
        c_xx = c_yy = None
        if not self.phase_only:
            amp = np.asarray(self.vals_amp)[g_start:g_stop]
            c_xx, c_yy = ev._upload(amp[..., 0]), ev._upload(amp[..., 1])
        fin = SF_EVAL_NAN_SCRUB | SF_EVAL_BIG_ENDIAN
        # with smoothing, scrub and byte swap come after the Gaussian
        # (screen.py:353-378 smooths, then replaces NaNs)
        flags = DEFAULT_FLAGS | fin if smooth_pix <= 0 else \
            DEFAULT_FLAGS & ~SF_EVAL_NAN_SCRUB

        def evaluate(r0, r1, buf):
            s = slice(r0 * slots, r1 * slots)
            out = buf.view(ev.torch.float32).view(-1, 4, ev.ny, ev.nx)
            if self.pol_phases:
                # 2 coefficient sets, 4 with the amplitudes
                ev.eval_pol_device(coef[s], coef_y[s], out,
                                   None if c_xx is None else c_xx[s],
                                   None if c_yy is None else c_yy[s], flags)
            elif self.phase_only:
                ev.eval_device(coef[s], out, flags)
            else:
                ev.eval_gain_device(coef[s], c_xx[s], c_yy[s], out, flags)
            if smooth_pix > 0:
                ev.smooth_device(out, smooth_pix, fin)

        stream_time_rows(writer, ev.dev, g_stop - g_start,
                         slots * 16 * ev.nx * ev.ny, max_batch_bytes, evaluate)

    def sampler(self):
        """The evaluator ``sample`` binds its positions on (no pixel grid)."""
        if self._sampler is None:
            self._sampler = KLEvaluator(self.piercepoints, self.r_0, self.beta_val,
                                        device=self.device)
        return self._sampler

    def sample(self, ra_deg, dec_deg, cellsize_deg=None, t_start=0, t_stop=None,
               values=False, max_batch_bytes=1 << 30):
        """The screens at sky positions, without building the cube.

        With ``cellsize_deg``: what the a-term cube of that cell size holds at
        the pixel containing each position (``geometry.patch_pixels``: the
        cube entry ``[..., iy, ix]``, i.e. the screen at ``(X[ix], Y[iy])`` of
        ``geometry.grid_coords``, Q8); positions outside the image give NaN
        columns.  Without it: the screen at the exact position
        (``geometry.screen_xy``).

        Returns float64 ``[t_stop - t_start, F, A, 4, P]`` -- the planes of
        ``make_matrix`` (raw, not NaN-scrubbed, float32 rounding) -- or, with
        ``values``, the phase screen itself ``[t_stop - t_start, F, A, P]`` in
        the fit's units (fp64).  With polarized phases (``pol_phases``) the
        positions are evaluated once per pol (two ``sf_kl_eval_points`` calls):
        planes 0 / 1 are those of the XX screens, planes 2 / 3 of the YY ones,
        and ``values`` carries a trailing pol axis ``[..., P, 2]``.  Runs in device batches of whole time rows of
        at most ``max_batch_bytes`` (coefficients + output), so the call's
        device footprint does not grow with the number of times."""
        ra = np.atleast_1d(np.asarray(ra_deg))
        de = np.atleast_1d(np.asarray(dec_deg))
        if ra.shape != de.shape or ra.ndim != 1:
            raise ValueError("ra_deg and dec_deg: equal-length 1-D arrays")
        n_pos = ra.shape[0]
        if cellsize_deg is None:
            x, y = geometry.screen_xy(ra, de, self.mid_ra, self.mid_dec)
            inside = np.isfinite(x) & np.isfinite(y)
        else:
            ix, iy, inside = geometry.patch_pixels(ra, de, self.rad, self.dec,
                                                   self.width_ra, cellsize_deg)
            gx, gy = geometry.grid_coords(self.rad, self.dec, self.width_ra,
                                          cellsize_deg, self.mid_ra, self.mid_dec)
            x = gx[np.where(inside, ix, 0)]
            y = gy[np.where(inside, iy, 0)]
        xy = np.stack([np.where(inside, x, 0.0), np.where(inside, y, 0.0)], axis=1)
        vals = np.asarray(self.vals_ph)
        n_t, n_f, n_a, D = vals.shape[:4]
        pols = 2 if self.pol_phases else 1
        t_stop = n_t if t_stop is None else min(int(t_stop), n_t)
        t_start = int(t_start)
        if not 0 <= t_start <= t_stop:
            raise ValueError(f"times [{t_start}, {t_stop}) outside 0..{n_t}")
        gain = not self.phase_only and not values
        shape = (t_stop - t_start, n_f, n_a) + ((n_pos,) if values else (4, n_pos))
        if values and self.pol_phases:
            shape += (2,)
        out = np.full(shape, np.nan)
        if t_stop == t_start or not inside.any():
            return out
        ev = self.sampler()
        flags = SF_EVAL_FAST_SINCOS  # raw planes: no NaN scrub (make_matrix)
        live = np.nonzero(inside)[0]
        for p0 in range(0, live.size, SF_MAX_POINTS):
            sel = live[p0:p0 + SF_MAX_POINTS]
            P = sel.size
            ev.set_points(xy[sel])
            row_bytes = n_f * n_a * ((8 if values else 16) * P * pols +
                                     8 * D * ((2 if gain else 0) + pols))
            rows = batch_rows(t_stop - t_start, row_bytes, max_batch_bytes)
            for t0 in range(t_start, t_stop, rows):
                t1 = min(t_stop, t0 + rows)
                dst = out[t0 - t_start:t1 - t_start]
                if gain:
                    amp = np.asarray(self.vals_amp)[t0:t1]
                    c_xx, c_yy = ev._upload(amp[..., 0]), ev._upload(amp[..., 1])
                for pol in range(pols):
                    coef = ev._upload(vals[t0:t1, ..., pol] if self.pol_phases
                                      else vals[t0:t1])
                    if values:
                        got = ev.sample_device(coef, values=True)
                    elif gain:
                        got = ev.sample_device(coef, c_xx, c_yy, flags=flags)
                    else:
                        got = ev.sample_device(coef, flags=flags)
                    got = got.cpu().numpy().reshape((t1 - t0, n_f, n_a) + got.shape[1:])
                    if not self.pol_phases:
                        dst[..., sel] = got
                    elif values:
                        dst[..., sel, pol] = got
                    else:
                        # the pol's own plane pair of its evaluation
                        dst[..., 2 * pol:2 * pol + 2, sel] = got[..., 2 * pol:2 * pol + 2, :]
                    del coef, got
        return out

    def patch_errors(self, cellsize_deg=None, max_batch_bytes=1 << 30):
        """The reference's acceptance quantity (tests/test_fit_screens.py,
        scripts/analyze_screens.py), per direction: float64 ``[D]``, the
        maximum over times, frequencies, stations and the four planes of
        |screen at the direction's position - expected|, where expected is
        (a_xx cos phi, a_xx sin phi, a_yy cos phi, a_yy sin phi), phi the input
        phase minus that of the reference station of ``fit`` and a the input
        amplitudes on the phase grid (1 for phase-only screens); with polarized
        phases planes 0 / 1 are compared with the XX input phases and planes
        2 / 3 with the YY ones, each referenced to the reference station.  Input
        entries with zero weight or a non-finite value are left out; a
        direction outside the image (``cellsize_deg`` given) or without any
        usable entry gives NaN.  Positions are those of the solset's source
        table; with ``cellsize_deg`` the screen is read at the pixel of the
        cube of that cell size, without it at the exact position.  Needs
        ``fit`` (``process``) on this object."""
        if self.solset is None:
            raise RuntimeError("patch_errors needs the input solutions: call "
                               "fit() or process() first")
        st = self.solset.get_soltab(self.input_phase_soltab_name)
        val = np.asarray(canonical_axes(st, st.val), np.float64)
        wgt = canonical_axes(st, st.weight)
        n_t, n_f, n_a, D = val.shape[:4]
        if not self.pol_phases:
            # one phase for both plane pairs: a pol axis of length 1 that views
            # the scalar arrays twice
            val, wgt = val[..., None], wgt[..., None]
        if not self.phase_only:
            sa = self.solset.get_soltab(self.input_amplitude_soltab_name)
            an = sa.get_axes_names()
            ao = [an.index(a) for a in ("time", "freq", "ant", "dir", "pol")]
            aval = np.transpose(np.asarray(sa.val, np.float64), ao)
            awgt = np.transpose(np.asarray(sa.weight), ao)
            # the input amplitudes on the phase grid: Screen.interpolate's
            # nearest-sample gather along time, then frequency
            from .screen import nearest_index
            if aval.shape[0] != n_t:
                it = (np.zeros(n_t, int) if aval.shape[0] == 1 else
                      nearest_index(np.asarray(sa.time), self.times_ph))
                aval, awgt = aval[it], awgt[it]
            if aval.shape[1] != n_f:
                jf = (np.zeros(n_f, int) if aval.shape[1] == 1 else
                      nearest_index(np.asarray(sa.freq), self.freqs_ph))
                aval, awgt = aval[:, jf], awgt[:, jf]
        src = np.asarray(self.source_positions, np.float32)
        ra, de = np.rad2deg(src[:, 0]), np.rad2deg(src[:, 1])  # float32 (Q11)
        if cellsize_deg is None:
            inside = np.ones(D, bool)
        else:
            inside = geometry.patch_pixels(ra, de, self.rad, self.dec,
                                           self.width_ra, cellsize_deg)[2]
        err = np.full(D, -np.inf)
        row_bytes = n_f * n_a * D * (16 + 8 * (1 if self.phase_only else 3))
        # host working set per time row: the sampled and the expected planes
        rows = max(1, int(max_batch_bytes // (row_bytes + n_f * n_a * D * 96)))
        for t0 in range(0, n_t, rows):
            t1 = min(n_t, t0 + rows)
            # position k is direction k's: the last axis of both arrays
            got = self.sample(ra, de, cellsize_deg, t0, t1,
                              max_batch_bytes=max_batch_bytes)
            phi = val[t0:t1] - val[t0:t1, :, self.ref_ind:self.ref_ind + 1]
            use = (wgt[t0:t1] != 0) & np.isfinite(val[t0:t1])
            if self.phase_only:
                axx = ayy = 1.0
            else:
                axx, ayy = aval[t0:t1, ..., 0], aval[t0:t1, ..., 1]
                use &= ((awgt[t0:t1, ..., 0] != 0) & (awgt[t0:t1, ..., 1] != 0) &
                        np.isfinite(axx) & np.isfinite(ayy))[..., None]
            px, py = phi[..., 0], phi[..., -1]  # the same array without pols
            want = (axx * np.cos(px), axx * np.sin(px),
                    ayy * np.cos(py), ayy * np.sin(py))
            for q in range(4):
                u = use[..., 0 if q < 2 else -1]
                diff = np.where(u, np.abs(got[:, :, :, q] - want[q]), -np.inf)
                err = np.maximum(err, diff.reshape(-1, D).max(axis=0))
        err[~inside | ~np.isfinite(err)] = np.nan
        return err
