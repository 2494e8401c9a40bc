"""Tessellated (Voronoi) screens of TEC solutions.

``VoronoiTecScreen`` is to ``VoronoiScreen`` what ``KLTecScreen`` is to
``KLScreen``: it renders a ``tec`` soltab (values in TECU) through the label
raster of the sky model, with no fit -- every pixel takes the value solved for
the direction whose cell contains it -- and writes either

* ``aterm_type="tec"``: the 5-axis cube of ``make_template_image(...,
  aterm_type="tec")`` (processing_utils.py:144-292), ``[time][freq][ant][y][x]``
  float32 dTEC values, filled by ``sf_tess_fill_values`` (csrc/tess_values.hip):
  one plane per slot, the optional Gaussian smoothing on the value images; or
* ``aterm_type="gain"``: the ordinary 6-axis Jones cube at given frequencies.
  The phases ``tec * tec_to_phase / nu (+ phi0)`` are built on the device per
  direction (``tess_gain_phases``) and go through ``sf_tess_fill`` like the
  phases of a ``VoronoiScreen``; smoothing then acts on the Jones planes.

The reference has no tessellated rendering of tec soltabs; its tessellated
path is the only one it allows for a one-direction solution set (Q14), which
``make_tec_aterm_image`` follows.  Weights are not consulted, as in
``VoronoiScreen``; a NaN value stays NaN until the cube's scrub.
"""

import numpy as np

from . import fits
from ._lib import SF_EVAL_BIG_ENDIAN, SF_EVAL_NAN_SCRUB, private_context
from .h5parm import H5parm, get_reference_station
from .kl_tec_screen import TEC_TO_PHASE, check_phase_soltab_axes, tec_to_phase_coef
from .screen import canonical_axes, nearest_index
from .streaming import stream_time_rows
from .voronoi_screen import VoronoiScreen


def tess_gain_phases(tec, freqs_tec, freqs_hz, tec_to_phase=TEC_TO_PHASE, phi0=None):
    """Per-direction phases of the gain cube: torch tensors ``tec`` (TECU) and
    ``phi0`` (radians or None), both [T, F_tec, A, D] on any device, ->
    [T, F, A, D] with ``out[:, f] = tec[:, i_f] * (tec_to_phase / freqs_hz[f])
    (+ phi0[:, i_f])``, i_f the TEC frequency nearest to ``freqs_hz[f]`` (0
    when there is only one)."""
    import torch

    n_f = len(freqs_hz)
    fidx = (np.zeros(n_f, np.int64) if tec.shape[1] == 1 else
            nearest_index(freqs_tec, freqs_hz))
    phase = tec_to_phase_coef(tec, freqs_hz, tec_to_phase, fidx)
    if phi0 is not None:
        idx = torch.as_tensor(np.asarray(fidx, np.int64), device=tec.device)
        phase = phase + phi0.index_select(1, idx)
    return phase


class VoronoiTecScreen(VoronoiScreen):
    """Tessellated screens of a ``tec`` soltab (values in TECU)."""

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
        self.vals_phi0 = None  # referenced, on the tec soltab's axes, radians
        self.ref_ind = None

    def fit(self):
        """Reference the dTEC values to one station, as ``VoronoiScreen.fit``
        references phases (the first station of largest summed weight among
        the first 10); with a phase soltab, its phases to the same station,
        broadcast over the tec frequencies when it has a single one."""
        self.vals_phi0 = None
        h5 = H5parm(self.input_h5parm_filename)
        solset = h5.get_solset(self.input_solset_name)
        st = solset.get_soltab(self.input_tec_soltab_name)
        if st.get_type() != "tec":
            raise ValueError(f"soltab {self.input_tec_soltab_name!r} of type "
                             f"{st.get_type()!r} cannot be fitted")
        names = list(st.get_axes_names())
        if sorted(names) != ["ant", "dir", "freq", "time"]:
            raise ValueError(f"soltab {self.input_tec_soltab_name!r}: axes {names}, "
                             "expected time, freq, ant and dir")
        ref = get_reference_station(st, 10)
        vals = np.array(canonical_axes(st, st.val), dtype=np.float64)
        self.vals_ph = vals - vals[:, :, ref:ref + 1]
        self.times_ph = np.asarray(st.time)
        self.freqs_ph = np.asarray(st.freq)
        self.vals_amp = None
        self.times_amp, self.freqs_amp = self.times_ph, self.freqs_ph
        if self.input_phi0_soltab_name is not None:
            sp = solset.get_soltab(self.input_phi0_soltab_name)
            if sp.get_type() != "phase":
                raise ValueError(f"soltab {self.input_phi0_soltab_name!r} of type "
                                 f"{sp.get_type()!r} is not a phase soltab")
            broadcast = check_phase_soltab_axes(st, sp)
            phi0 = np.array(canonical_axes(sp, sp.val), dtype=np.float64)
            phi0 = phi0 - phi0[:, :, ref:ref + 1]
            if broadcast:
                phi0 = np.repeat(phi0, len(self.freqs_ph), axis=1)
            self.vals_phi0 = phi0
        self.ref_ind = ref
        self.source_names = st.dir
        self.source_dict = solset.get_source()
        self.source_positions = [self.source_dict[s] for s in self.source_names]
        self.station_names = st.ant
        self.station_dict = solset.get_ant()
        self.station_positions = [self.station_dict[s] for s in self.station_names]
        h5.close()

    def get_memory_usage(self, cellsize_deg, aterm_type="tec", n_freq=None):
        """GB per time slot, ``VoronoiScreen``'s estimate (x10 overhead) for a
        [1, F, A, ny, nx] array ("gain": [1, F, A, 4, ny, nx])."""
        ximsize = int(self.width_ra / cellsize_deg)
        yimsize = int(self.width_dec / cellsize_deg)
        n_freq = len(self.freqs_ph) if n_freq is None else n_freq
        planes = 4 if aterm_type == "gain" else 1
        nbytes = 8 * n_freq * len(self.station_names) * planes * yimsize * ximsize
        return nbytes / 1024 ** 3 * 10

    def values_device(self, vals_dev, out_dev, smooth_pix=0.0, flags=SF_EVAL_NAN_SCRUB):
        """device [S, D] referenced values -> device [S, ny, nx] float32
        (``sf_tess_fill_values``), on a context of its own, as
        ``eval_device``."""
        import torch
        dev, lab = self._device()
        ny, nx = self.data_rasertize_template.shape
        S, D = vals_dev.shape
        with private_context(self.device) as ctx, torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            busy = getattr(ctx, "tess_busy", None)
            if busy is not None:
                stream.wait_event(busy)
            ctx.set_stream(stream.cuda_stream)
            ctx.tess_fill_values(lab, nx, ny, vals_dev, D, S, out_dev,
                                 smooth_pix=smooth_pix, flags=flags)
            ctx.tess_busy = torch.cuda.Event()
            ctx.tess_busy.record(stream)
        return out_dev

    def values_host(self, values, smooth_pix=0.0, flags=SF_EVAL_NAN_SCRUB):
        """[..., D] referenced values -> float32 [..., ny, nx] (gather +
        optional Gaussian smoothing) on the GPU."""
        import torch
        dev, _ = self._device()
        lead = np.shape(values)[:-1]
        ny, nx = self.data_rasertize_template.shape
        v = self._upload(values)
        out = torch.empty((v.shape[0], ny, nx), dtype=torch.float32, device=dev)
        self.values_device(v, out, smooth_pix, flags)
        return out.cpu().numpy().reshape(lead + (ny, nx))

    def make_matrix(self, t_start_index, t_stop_index, freq_ind, stat_ind,
                    cellsize_deg, out_dir=None, ncpu=0, aterm_type="tec"):
        """(t_stop - t_start, ny, nx) float64: the dTEC image of one
        (frequency, station), NaN where the value is NaN, with the float32
        rounding of the cube.  ``out_dir`` is needed only while the template
        has not been made."""
        del ncpu
        if aterm_type != "tec":
            raise ValueError('make_matrix renders aterm_type "tec" only')
        if self.data_rasertize_template is None:
            self.make_rasertize_template(cellsize_deg, out_dir)
        vals = self.vals_ph[t_start_index:t_stop_index, freq_ind, stat_ind]
        return self.values_host(vals, flags=0).astype(np.float64)

    def _upload4(self, a):
        import torch
        dev, _ = self._device()
        return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)

    def write_chunk(self, writer, g_start, g_stop, cellsize_deg, smooth_pix,
                    max_batch_bytes=1 << 30):
        """dTEC images of times [g_start, g_stop), all (freq, station), in
        FITS byte order, NaN-scrubbed after the smoothing on the device,
        streamed through pinned buffers (see streaming.py)."""
        import torch
        dev, _ = self._device()
        ny, nx = self.data_rasertize_template.shape
        vals = self.vals_ph[g_start:g_stop]
        slots = vals.shape[1] * vals.shape[2]  # per time row
        v = self._upload(vals)

        def evaluate(r0, r1, buf):
            out = buf.view(torch.float32).view(-1, ny, nx)
            self.values_device(v[r0 * slots:r1 * slots], out, smooth_pix,
                               SF_EVAL_NAN_SCRUB | SF_EVAL_BIG_ENDIAN)

        stream_time_rows(writer, dev, g_stop - g_start, slots * 4 * nx * ny,
                         max_batch_bytes, evaluate)

    def write_chunk_gain(self, writer, g_start, g_stop, cellsize_deg, smooth_pix,
                         freqs_hz, tec_to_phase, max_batch_bytes=1 << 30):
        """Jones planes (cos, sin, cos, sin) of the phase tec_to_phase / nu x
        dTEC (+ the phase soltab's, when the object has one) at ``freqs_hz``,
        times [g_start, g_stop): the phases per direction on the device, then
        the fill of ``VoronoiScreen`` (smoothing on the Jones planes)."""
        import torch
        dev, _ = self._device()
        ny, nx = self.data_rasertize_template.shape
        tec = self._upload4(self.vals_ph[g_start:g_stop])
        phi0 = None
        if self.vals_phi0 is not None:
            phi0 = self._upload4(self.vals_phi0[g_start:g_stop])
        n_f, n_a, D = len(freqs_hz), tec.shape[2], tec.shape[3]

        def evaluate(r0, r1, buf):
            phase = tess_gain_phases(tec[r0:r1], self.freqs_ph, freqs_hz, tec_to_phase,
                                     None if phi0 is None else phi0[r0:r1])
            out = buf.view(torch.float32).view(-1, 4, ny, nx)
            self.eval_device(phase.reshape(-1, D), out, smooth_pix,
                             SF_EVAL_NAN_SCRUB | SF_EVAL_BIG_ENDIAN)

        stream_time_rows(writer, dev, g_stop - g_start, n_f * n_a * 16 * nx * ny,
                         max_batch_bytes, evaluate)

    def write(self, out_dir, cellsize_deg, smooth_pix=0, aterm_type="tec",
              tec_to_phase=TEC_TO_PHASE, freqs_hz=None, ncpu=0):
        """Write ``{name}_{g}.fits`` per time chunk, ``{name}.txt`` listing
        them and ``{name}_template.fits``.

        ``aterm_type="tec"``: the 5-axis dTEC cube [time][freq][ant][y][x] on
        the soltab's frequency axis, ``smooth_pix`` applied to the value
        images.  ``aterm_type="gain"``: the 6-axis Jones cube at ``freqs_hz``
        (default: the soltab's), phase = ``tec_to_phase`` x dTEC / nu (+ the
        phase soltab's); with several tec frequencies each output frequency
        takes the nearest one's values; ``smooth_pix`` acts on the Jones
        planes, as for phase screens.  ``tec_to_phase`` (rad Hz / TECU) is the
        imager-side convention (see ``kl_tec_screen``)."""
        if aterm_type not in ("tec", "gain"):
            raise ValueError(f"unknown aterm_type {aterm_type!r}")
        self.ncpu = ncpu
        if self.data_rasertize_template is None:
            self.make_rasertize_template(cellsize_deg, out_dir)
        gain = aterm_type == "gain"
        freqs = np.asarray(self.freqs_ph if freqs_hz is None or not gain else freqs_hz,
                           np.float64).reshape(-1)
        mem = self.get_memory_usage(cellsize_deg, aterm_type, len(freqs))
        if gain:
            return self._write_cubes(
                out_dir, cellsize_deg, mem, fits.aterm_header, freqs, (4,),
                lambda writer, g_start, g_stop: self.write_chunk_gain(
                    writer, g_start, g_stop, cellsize_deg, smooth_pix, freqs,
                    tec_to_phase))
        return self._write_cubes(
            out_dir, cellsize_deg, mem, fits.tec_header, freqs, (),
            lambda writer, g_start, g_stop: self.write_chunk(
                writer, g_start, g_stop, cellsize_deg, smooth_pix))
