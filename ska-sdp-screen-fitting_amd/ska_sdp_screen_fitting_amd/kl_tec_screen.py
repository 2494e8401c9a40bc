"""KL screens fitted to TEC solutions, rendered as the dTEC a-term cube.

``KLTecScreen`` fits a ``tec`` soltab with ``stationscreen.run`` (the
reference fits tec soltabs, stationscreen.py:858-1161, but has no screen class
that renders them) and writes either

* ``aterm_type="tec"``: the 5-axis cube of ``make_template_image(...,
  aterm_type="tec")`` (processing_utils.py:144-292, its default layout):
  ``[time][freq][ant][y][x]`` float32 dTEC values, no MATRIX axis -- the cube
  an imager turns into phases itself, per channel.  The values come from
  ``sf_kl_eval_values`` (csrc/kl_values.hip): fp64 contraction, one cast; or
* ``aterm_type="gain"``: the ordinary 6-axis Jones cube at given frequencies.
  The KL map is linear, so the phase screen at frequency nu is the screen of
  the coefficients ``tec_coef * tec_to_phase / nu``.  Two paths render it
  (keyword ``fused``): the replicated one -- one broadcast on the device, then
  ``sf_kl_eval`` over T x F x A slots -- and the fused one, ``sf_kl_eval_tec``
  (csrc/kl_tec.hip): one contraction per (time, station), the scale and the
  cos / sin per channel, no per-channel coefficients on the device.

With ``phase_soltab_name`` (LOFAR-style ``tecandphase`` solutions: a tec soltab
and a frequency-independent scalar-phase soltab over the same directions) the
gain cube renders ``exp(i (phi0 + tec_to_phase * dTEC / nu))``.
"""

import os

import numpy as np

from . import fits
from . import stationscreen
from ._lib import SF_EVAL_BIG_ENDIAN, SF_EVAL_NAN_SCRUB
from .h5parm import H5parm, get_reference_station
from .kl_screen import DEFAULT_FLAGS, KLBase
from .screen import nearest_index
from .streaming import stream_time_rows

# phase [rad] = TEC_TO_PHASE * dTEC [TECU] / nu [Hz]: -8.4479745e9 is the usual
# first-order ionospheric constant (-e^2 / (4 pi eps0 m_e c) * 1e16).  It is
# NOT taken from the reference, which never converts tec screens to phases:
# the imager's own convention decides, so every caller below takes it as a
# parameter.
TEC_TO_PHASE = -8.4479745e9


def tec_to_phase_coef(tec_coef, freqs_hz, tec_to_phase=TEC_TO_PHASE,
                      freq_index=None):
    """Phase-screen coefficients of TEC-screen coefficients: torch tensor
    ``tec_coef`` [T, F_tec, A, D] (any device) -> [T, F, A, D] with
    ``out[:, f] = tec_coef[:, freq_index[f]] * tec_to_phase / freqs_hz[f]``.
    ``freq_index`` defaults to 0 for every f (one tec frequency) and must be
    given when the soltab has more."""
    import torch

    nu = torch.as_tensor(np.asarray(freqs_hz, np.float64), device=tec_coef.device)
    if freq_index is None:
        if tec_coef.shape[1] != 1:
            raise ValueError("freq_index: needed for more than one tec frequency")
        src = tec_coef  # [T, 1, A, D] x [F] -> [T, F, A, D]
    else:
        idx = torch.as_tensor(np.asarray(freq_index, np.int64), device=tec_coef.device)
        src = tec_coef.index_select(1, idx)
    return (src * (tec_to_phase / nu)[None, :, None, None]).contiguous()


# fused="auto": the (D, F) region where sf_kl_eval_tec beat tec_to_phase_coef +
# sf_kl_eval by more than the latter's max - min spread, measured by
# tools/eval_tec.py at 256^2 (profiles/eval_tec.txt: D in {20, 50, 61, 80, 128}
# x F in {1, 8, 32}).  It won every shape above 60 directions, where sf_kl_eval
# runs the fp64 wide kernel (x1.04-1.05 at F = 1, x1.3-2.3 at F = 8 and 32),
# and none at D = 20 and 50, where the LDS-staged and integer-digit kernels of
# sf_kl_eval stay ahead or level.  Between measured points the rule takes the
# nearest measured point at or below in both D and F; below the smallest
# measured D or F it is the replicated path.
FUSED_AUTO_D = (20, 50, 61, 80, 128)
FUSED_AUTO_F = (1, 8, 32)
# FUSED_AUTO_WINS[i][j]: fused won at D = FUSED_AUTO_D[i], F = FUSED_AUTO_F[j]
FUSED_AUTO_WINS = ((False, False, False),
                   (False, False, False),
                   (True, True, True),
                   (True, True, True),
                   (True, True, True))


def fused_auto(n_dir, n_freq):
    """The ``fused="auto"`` rule: True where the measured table says the fused
    evaluation wins for ``n_dir`` directions and ``n_freq`` output channels."""
    i = int(np.searchsorted(FUSED_AUTO_D, n_dir, side="right")) - 1
    j = int(np.searchsorted(FUSED_AUTO_F, n_freq, side="right")) - 1
    return i >= 0 and j >= 0 and FUSED_AUTO_WINS[i][j]


def check_phase_soltab_axes(soltab_tec, soltab_phase):
    """The phase soltab of a tecandphase solution must lie on the tec soltab's
    grid: axes time, freq, ant, dir (no pol), the tec soltab's times, stations
    and directions, and its frequencies or a single one.  Raises ValueError
    naming the axis that differs; returns True when the phase soltab's
    length-1 frequency axis has to be broadcast over the tec soltab's."""
    names = list(soltab_phase.get_axes_names())
    if sorted(names) != ["ant", "dir", "freq", "time"]:
        raise ValueError(f"phase soltab: axes {names}, expected time, freq, ant "
                         "and dir (a scalar phase, no pol axis)")
    for axis in ("time", "ant", "dir"):
        a, b = np.asarray(getattr(soltab_tec, axis)), np.asarray(getattr(soltab_phase, axis))
        same = a.shape == b.shape and (
            np.array_equal(a, b) if axis == "time" else
            [str(x) for x in a] == [str(x) for x in b])
        if not same:
            raise ValueError(f"phase soltab: its {axis} axis differs from the tec "
                             f"soltab's ({b.shape[0]} against {a.shape[0]} entries"
                             f"{'' if a.shape != b.shape else ', other values'})")
    fa, fb = np.asarray(soltab_tec.freq, np.float64), np.asarray(soltab_phase.freq, np.float64)
    if np.array_equal(fa, fb):
        return False
    if fb.shape == (1,):
        return True
    raise ValueError("phase soltab: its freq axis differs from the tec soltab's "
                     f"({fb.shape[0]} against {fa.shape[0]} entries) and is not of "
                     "length 1")


class KLTecScreen(KLBase):
    """KL screens of a ``tec`` soltab (values in TECU)."""

    def __init__(self, name, h5parm_filename, skymodel_filename, rad, dec,
                 width_ra, width_dec, solset_name="sol000",
                 tec_soltab_name="tec000", phase_soltab_name=None):
        super().__init__(name, h5parm_filename, skymodel_filename, rad, dec,
                         width_ra, width_dec, solset_name=solset_name,
                         phase_soltab_name=tec_soltab_name,
                         amplitude_soltab_name=None)
        self.input_tec_soltab_name = tec_soltab_name
        # the frequency-independent scalar phase of a tecandphase solution
        self.input_phi0_soltab_name = phase_soltab_name
        self.vals_phi0 = None  # its screens on tec_screen000's axes, radians

    def fit(self):
        """Fit the tec screens as ``KLScreen.fit`` fits phases: reference
        station among the first 10, order min(20, D - 1) scaled per station.
        With a phase soltab, its screens too, same reference station and
        order rule (``phase_screen000``)."""
        self._evaluators = {}
        self.vals_phi0 = None
        h5 = H5parm(self.input_h5parm_filename)
        solset = h5.get_solset(self.input_solset_name)
        soltab_tec = solset.get_soltab(self.input_tec_soltab_name)
        dirs = [str(d) for d in soltab_tec.dir]
        self._check_sky_model(dirs)
        ref_ind = get_reference_station(soltab_tec, 10)
        screen_order = min(20, len(dirs) - 1)
        rc = stationscreen.run(soltab_tec, "tec_screen000", order=screen_order,
                               ref_ant=ref_ind, scale_order=True, adjust_order=True,
                               ncpu=self.ncpu or 0, device=self.device)
        if rc != 0:
            raise ValueError(f"soltab {self.input_tec_soltab_name!r} of type "
                             f"{soltab_tec.get_type()!r} cannot be fitted")
        if self.input_phi0_soltab_name is not None:
            soltab_phi0 = solset.get_soltab(self.input_phi0_soltab_name)
            if soltab_phi0.get_type() != "phase":
                raise ValueError(f"soltab {self.input_phi0_soltab_name!r} of type "
                                 f"{soltab_phi0.get_type()!r} is not a phase soltab")
            broadcast = check_phase_soltab_axes(soltab_tec, soltab_phi0)
            stationscreen.run(soltab_phi0, "phase_screen000", order=screen_order,
                              ref_ant=ref_ind, scale_order=True, adjust_order=True,
                              ncpu=self.ncpu or 0, device=self.device)
            phi0 = np.asarray(solset.get_soltab("phase_screen000").val, np.float64)
            if broadcast:
                phi0 = np.repeat(phi0, len(soltab_tec.freq), axis=1)
            self.vals_phi0 = phi0
        st = solset.get_soltab("tec_screen000")
        # (vals_ph / times_ph / freqs_ph: the names Screen.write's chunking reads)
        self.vals_ph = st.val
        self._adopt_screen_soltab(st, solset)
        self.ref_ind = ref_ind
        h5.close()

    def get_memory_usage(self, cellsize_deg, aterm_type="tec", n_freq=None):
        """GB per time slot (``_memory_usage``) for a [1, F, A, ny, nx] array
        ("gain": [1, F, A, 4, ny, nx])."""
        return self._memory_usage(
            cellsize_deg, len(self.freqs_ph) if n_freq is None else n_freq,
            4 if aterm_type == "gain" else 1)

    def make_matrix(self, t_start_index, t_stop_index, freq_ind, stat_ind,
                    cellsize_deg, out_dir=None, ncpu=0, aterm_type="tec"):
        """(t_stop - t_start, ny, nx) float64: the dTEC screen of one
        (frequency, station), NaN where a coefficient is NaN, with the float32
        rounding of the cube (Q12)."""
        del out_dir, ncpu
        if aterm_type != "tec":
            raise ValueError('make_matrix renders aterm_type "tec" only')
        coef = np.asarray(self.vals_ph)[t_start_index:t_stop_index, freq_ind, stat_ind, :]
        return self.evaluator(cellsize_deg).values_host(coef).astype(np.float64)

    def write_chunk(self, writer, g_start, g_stop, cellsize_deg,
                    max_batch_bytes=1 << 30):
        """dTEC values of times [g_start, g_stop), all (freq, station): device
        batches of whole time rows in FITS byte order, NaN-scrubbed on the
        device, streamed through pinned buffers (as KLScreen.write_chunk)."""
        ev = self.evaluator(cellsize_deg)
        vals = np.asarray(self.vals_ph)[g_start:g_stop]
        slots = vals.shape[1] * vals.shape[2]  # per time row
        coef = ev._upload(vals)
        flags = SF_EVAL_NAN_SCRUB | SF_EVAL_BIG_ENDIAN

        def evaluate(r0, r1, buf):
            out = buf.view(ev.torch.float32).view(-1, ev.ny, ev.nx)
            ev.values_device(coef[r0 * slots:r1 * slots], out, flags)

        stream_time_rows(writer, ev.dev, g_stop - g_start,
                         slots * 4 * ev.nx * ev.ny, max_batch_bytes, evaluate)

    def write_chunk_gain(self, writer, g_start, g_stop, cellsize_deg, freqs_hz,
                         tec_to_phase, max_batch_bytes=1 << 30, fused="auto"):
        """Jones planes (cos, sin, cos, sin) of the phase tec_to_phase / nu x
        dTEC (+ the phase soltab's screens, when the object has one) at
        ``freqs_hz``, times [g_start, g_stop).

        ``fused=False``: the coefficients replicated and scaled per channel
        (``tec_to_phase_coef``, plus the phase coefficients: the KL map is
        linear and the piercepoints are shared), then ``sf_kl_eval``.
        ``fused=True``: the TEC (and phase) coefficients uploaded once,
        ``sf_kl_eval_tec`` per batch.  ``"auto"``: ``fused_auto(D, F)``."""
        if fused not in (False, True, "auto"):
            raise ValueError(f'fused: {fused!r}, expected False, True or "auto"')
        ev = self.evaluator(cellsize_deg)
        torch = ev.torch
        vals = np.asarray(self.vals_ph)[g_start:g_stop]
        n_a, D = vals.shape[2], vals.shape[3]
        n_f = len(freqs_hz)
        if fused == "auto":
            fused = fused_auto(D, n_f)
        fidx = (np.zeros(n_f, int) if vals.shape[1] == 1 else
                nearest_index(self.freqs_ph, freqs_hz))
        tec = ev._upload(vals, vals.shape)
        phi0 = None
        if self.vals_phi0 is not None:
            phi0 = np.asarray(self.vals_phi0)[g_start:g_stop]
            phi0 = ev._upload(phi0, phi0.shape)
        flags = DEFAULT_FLAGS | SF_EVAL_NAN_SCRUB | SF_EVAL_BIG_ENDIAN
        rad_per_tecu = tec_to_phase / np.asarray(freqs_hz, np.float64)
        idx = torch.as_tensor(np.asarray(fidx, np.int64), device=ev.dev)

        def evaluate(r0, r1, buf):
            sl = slice(r0, r1)
            if fused:
                out = buf.view(torch.float32).view(r1 - r0, n_f, n_a, 4, ev.ny, ev.nx)
                ev.eval_tec_device(tec[sl], rad_per_tecu, fidx,
                                   None if phi0 is None else phi0[sl], out, flags)
            else:
                coef = tec_to_phase_coef(tec[sl], freqs_hz, tec_to_phase, fidx)
                if phi0 is not None:
                    coef = coef + phi0[sl].index_select(1, idx)
                out = buf.view(torch.float32).view(-1, 4, ev.ny, ev.nx)
                ev.eval_device(coef.view(-1, D), out, flags)

        stream_time_rows(writer, ev.dev, g_stop - g_start,
                         n_f * n_a * 16 * ev.nx * ev.ny, max_batch_bytes, evaluate)

    def write(self, out_dir, cellsize_deg, aterm_type="tec",
              tec_to_phase=TEC_TO_PHASE, freqs_hz=None, ncpu=0, fused="auto"):
        """Write ``{name}_{g}.fits`` per time chunk (Screen.write's gap and
        memory chunking) and ``{name}.txt`` listing them.

        ``aterm_type="tec"``: the 5-axis dTEC cube [time][freq][ant][y][x] on
        the soltab's frequency axis.  ``aterm_type="gain"``: the 6-axis Jones
        cube at ``freqs_hz`` (default: the soltab's), phase = ``tec_to_phase``
        x dTEC / nu; with several tec frequencies each output frequency takes
        the nearest one's screens.  ``tec_to_phase`` (rad Hz / TECU) is the
        imager-side convention, not something the reference defines: check it
        against the consumer of the cube.  With a phase soltab the gain cube
        renders phi0 + tec_to_phase x dTEC / nu; ``aterm_type="tec"`` ignores
        it.  ``fused`` (``False``, ``True`` or ``"auto"``) picks the gain
        cube's evaluation, see ``write_chunk_gain``."""
        if aterm_type not in ("tec", "gain"):
            raise ValueError(f"unknown aterm_type {aterm_type!r}")
        self.ncpu = ncpu
        gain = aterm_type == "gain"
        freqs = np.asarray(self.freqs_ph if freqs_hz is None or not gain else freqs_hz,
                           np.float64).reshape(-1)
        mem = self.get_memory_usage(cellsize_deg, aterm_type, len(freqs))
        if gain:
            return self._write_cubes(
                out_dir, cellsize_deg, mem, fits.aterm_header, freqs, (4,),
                lambda writer, g_start, g_stop: self.write_chunk_gain(
                    writer, g_start, g_stop, cellsize_deg, freqs, tec_to_phase,
                    fused=fused))
        return self._write_cubes(
            out_dir, cellsize_deg, mem, fits.tec_header, freqs, (),
            lambda writer, g_start, g_stop: self.write_chunk(
                writer, g_start, g_stop, cellsize_deg))


def make_tec_aterm_image(h5parmfile, soltabname="tec000", outroot="",
                         bounds_deg=None, bounds_mid_deg=None, skymodel=None,
                         solsetname="sol000", padding_fraction=1.4,
                         cellsize_deg=0.2, aterm_type="tec", ncpu=0,
                         tec_to_phase=TEC_TO_PHASE, freqs_hz=None, fused="auto",
                         phase_soltab_name=None, screen_type="kl", smooth_deg=0):
    """``make_aterm_image`` for a tec soltab: fit KL screens to it and write
    the dTEC cube (``aterm_type="tec"``) or the Jones cube at ``freqs_hz``
    (``"gain"``, see ``KLTecScreen.write`` for ``tec_to_phase`` and ``fused``).
    ``phase_soltab_name``: the scalar-phase soltab of a tecandphase solution,
    added to the gain cube's phase.  ``screen_type="tessellated"`` renders the
    solved values through the sky model's Voronoi cells instead
    (``VoronoiTecScreen``; ``fused`` does not apply), smoothed by a Gaussian
    of ``smooth_deg``; "kl" ignores ``smooth_deg``, and a soltab with one
    direction is always tessellated -- both as ``make_aterm_image`` (Q14).
    Bounds and padding as ``make_aterm_image``.  Returns None."""
    from .make_aterm_images import padded_bounds
    if screen_type not in ("kl", "tessellated"):
        raise ValueError(f"unknown screen_type {screen_type!r}")
    bounds_deg, bounds_mid_deg = padded_bounds(bounds_deg, bounds_mid_deg,
                                               padding_fraction)
    cellsize_deg = float(cellsize_deg)
    width_deg = bounds_deg[3] - bounds_deg[1]
    # one direction forces the tessellated screen (Q14)
    h5 = H5parm(h5parmfile)
    if len(h5.get_solset(solsetname).get_soltab(soltabname).dir) == 1:
        screen_type = "tessellated"
    h5.close()
    if screen_type == "tessellated":
        from .voronoi_tec_screen import VoronoiTecScreen
        screen = VoronoiTecScreen(os.path.basename(outroot), h5parmfile, skymodel,
                                  bounds_mid_deg[0], bounds_mid_deg[1], width_deg,
                                  width_deg, solset_name=solsetname,
                                  tec_soltab_name=soltabname,
                                  phase_soltab_name=phase_soltab_name)
        screen.process(ncpu=ncpu)
        screen.write(os.path.dirname(outroot), cellsize_deg,
                     smooth_pix=float(smooth_deg) / cellsize_deg, aterm_type=aterm_type,
                     tec_to_phase=tec_to_phase, freqs_hz=freqs_hz, ncpu=ncpu)
        return
    screen = KLTecScreen(os.path.basename(outroot), h5parmfile, skymodel,
                         bounds_mid_deg[0], bounds_mid_deg[1], width_deg, width_deg,
                         solset_name=solsetname, tec_soltab_name=soltabname,
                         phase_soltab_name=phase_soltab_name)
    screen.process(ncpu=ncpu)
    screen.write(os.path.dirname(outroot), cellsize_deg, aterm_type=aterm_type,
                 tec_to_phase=tec_to_phase, freqs_hz=freqs_hz, ncpu=ncpu, fused=fused)
