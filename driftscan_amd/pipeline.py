"""PipelineManager: one YAML file that takes telescope timestreams to KL modes, power spectra and maps.

The counterpart of ``drift.pipeline.pipeline.PipelineManager`` (drift/pipeline/pipeline.py:20-198), by behaviour: the same
sections — ``config`` (the properties below), ``timestreams`` (entries with ``name``, ``directory``, optionally
``output_directory``, ``mmode_ridge`` (this package: the ridge of the weighted m-modes of flagged data),
``flag_noise_bias_correct`` (this package: ``powerspectrum`` also subtracts the noise bias the flags add) and a ``simulate``
block of arguments for ``timestream.simulate`` plus its ``product_directory``;
the files of its ``maps`` and ``sources`` lists go through ``fixpath``; with ``unstacked: true`` the block goes to
``timestream.simulate_unstacked`` instead — one realisation of the device route of ``simulate_ensemble``, one row per feed
pair; such an entry is kept in ``unstacked``, apart from the timestreams the stages run on — and an entry with
``stack_from: {directory, calibrate: file|none|redundant|model, redcal: {...}, modelcal: {...}, dead_feeds: [...]}`` is
made from such a directory by ``timestream.stack_baselines`` before the m-modes, when its own directory does not exist
yet; ``redcal`` holds the solver's ``damping``, ``tol``, ``maxiter`` and ``reference`` (``file``, ``model`` or absent) of
``calibrate: redundant``; ``modelcal`` holds the ``model`` (a stacked timestream directory, through ``fixpath``),
``interval``, ``damping``, ``tol``, ``maxiter``, ``edge_floor`` and ``min_model`` of ``calibrate: model`` and of
``reference: model``)
and optionally ``crosspower`` (entries with ``psname``, ``klname``, ``timestreams``, ``psfile``) — the same defaults,
exceptions and methods.  Two deliberate differences:

* ``timestreams`` and ``simulations`` belong to the instance.  The reference keeps them as class attributes, so every
  PipelineManager of a process shares (and keeps adding to) one dictionary.
* the cross-power block selects the power-spectrum estimator ``psname`` on its timestreams.  The reference passes
  ``klname`` to ``set_psestimator`` there, which only works when the two names coincide.

One knob of this package: ``batched`` (default True) runs the m-mode chain and the a_lm stage of the SVD / KL map-makers
in device batches (``Timestream.generate_modes_batched``, ``mapmake_svd_batched``, ``mapmake_kl_batched``); False runs the
per-m methods.  Both write the same files.  And one list beside ``klmaps``: ``catalogues``, entries ``{name, file, source:
svd | <klname>, wiener, stack: {halfwidth, ...}}``, each of which writes ``spectra_<name>.hdf5`` per timestream in the maps
stage — the spectrum of the estimated sky at every position of the catalogue ``file`` and, when the catalogue carries
redshifts, their stack (``Timestream.catalogue_spectra``; needs ``batched``).  The default ``[]`` changes nothing.
And ``ringmaps``, entries ``{name, nel, weighting: natural | uniform, window: hann | blackman, ew: [...], intracyl, parts,
collapse_ew}`` (all optional), each of which writes ``ringmap_<name>.hdf5`` per frequency and at the root of every timestream
in the maps stage: its stacked visibilities beamformed north-south, sample by sample (``timestream.ringmap``).  It needs no
products beyond the telescope; an unknown key raises ValueError.
And ``delayspectra``, entries ``{name, nd, oversample, tau_max, taper, weighting: mask | weight, norm: window | inverse, ridge,
min_valid, tbin, blen_bins}`` (all optional), each of which writes ``delayspectrum_<name>.hdf5`` at the root of every
timestream in the maps stage: the delay power spectrum of every stacked baseline with its window function
(``timestream.delay_spectrum``); an unknown key raises ValueError.
And ``formedbeams``, entries ``{name, catalogue, ha_max, envelope_fwhm, weighting, window, ew: [...], intracyl, parts, stack:
{halfwidth, line_mhz, source_weight, channel_weight}}`` (``catalogue``, a file of positions, is required), each of which
writes ``formedbeam_<name>.hdf5`` per frequency and at the root of every timestream in the maps stage: a tracking beam
formed on every catalogue position from the stacked visibilities, one spectrum per object and class pair, and with
redshifts in the catalogue their stack (``timestream.formed_beam``).  It needs no products beyond the telescope either.

    python -m driftscan_amd.pipeline params.yaml
"""
import argparse
import logging
import os

import yaml

from . import config, manager, timestream

logger = logging.getLogger(__name__)


def fixpath(path):
    """`~`, environment variables and redundant separators resolved."""
    return os.path.normpath(os.path.expandvars(os.path.expanduser(path)))


class PipelineManager(config.Reader):
    product_directory = config.Property(proptype=str, default="")

    generate_modes = config.Property(proptype=bool, default=True)
    generate_klmodes = config.Property(proptype=bool, default=True)
    generate_powerspectra = config.Property(proptype=bool, default=True)
    generate_maps = config.Property(proptype=bool, default=True)

    no_m_zero = config.Property(proptype=bool, default=True)

    klmodes = config.Property(proptype=list, default=[])
    powerspectra = config.Property(proptype=list, default=[])
    klmaps = config.Property(proptype=list, default=[])
    # spectra at catalogue positions and their stack (not in the reference): entries {name, file, source: svd | <klname>,
    # wiener, stack: {halfwidth, line_mhz, source_weight, channel_weight}}; run in the maps stage when `batched` is on
    catalogues = config.Property(proptype=list, default=[])
    # ring maps (not in the reference): entries {name, nel, weighting, window, ew, intracyl, parts, collapse_ew}
    ringmaps = config.Property(proptype=list, default=[])
    # formed beams on catalogue positions (not in the reference): entries {name, catalogue, ha_max, envelope_fwhm, weighting,
    # window, ew, intracyl, parts, stack}
    formedbeams = config.Property(proptype=list, default=[])
    # delay power spectra (not in the reference): entries {name, nd, oversample, tau_max, taper, weighting, norm, ridge,
    # min_valid, tbin, blen_bins}
    delayspectra = config.Property(proptype=list, default=[])

    nside = config.Property(proptype=int, default=128)
    wiener = config.Property(proptype=bool, default=False)

    collect_klmodes = config.Property(proptype=bool, default=True)

    # device route of the m-mode chain and the map-makers (not in the reference)
    batched = config.Property(proptype=bool, default=True)
    chunk_gb = config.Property(proptype=float, default=4.0)

    manager = None

    def __init__(self):
        self.timestreams = {}
        self.simulations = {}
        self.stacks = {}
        self.unstacked = {}
        self.sidereal = {}
        self.days = {}
        self.crosspower = []

    @classmethod
    def from_configfile(cls, configfile):
        c = cls()
        c.load_configfile(configfile)
        return c

    def load_configfile(self, configfile):
        with open(configfile, "r") as f:
            yconf = yaml.safe_load(f)
        if not yconf or "config" not in yconf:
            raise Exception("Configuration file must have an 'config' section.")
        self.read_config(yconf["config"])
        for entry in self.ringmaps:   # an unknown key is refused before anything runs
            timestream.ringmap_params(entry)
        for entry in self.delayspectra:
            timestream.delayspectrum_params(entry)
        for entry in self.formedbeams:
            if timestream.formedbeam_params(entry)["catalogue"] is None:
                raise ValueError("formedbeams: an entry needs `catalogue`, a file of positions")
        self.product_directory = fixpath(self.product_directory) if self.product_directory else self.product_directory
        if "timestreams" not in yconf:
            raise Exception("Configuration file must have an 'timestream' section.")
        for tsconf in yconf["timestreams"]:
            ts = timestream.Timestream(fixpath(tsconf["directory"]), self._products(self.product_directory))
            if "output_directory" in tsconf:
                ts.output_directory = fixpath(tsconf["output_directory"])
            ts.no_m_zero = self.no_m_zero
            if "mmode_ridge" in tsconf:   # Tikhonov term of the weighted m-modes of flagged data
                ts.mmode_ridge = float(tsconf["mmode_ridge"])
            if "flag_noise_bias_correct" in tsconf:   # powerspectrum() subtracts the noise bias of the flags too
                ts.flag_noise_bias_correct = bool(tsconf["flag_noise_bias_correct"])
            if (tsconf.get("simulate") or {}).get("unstacked", False):
                # per-feed-pair data: the input of another entry's `stack_from`, not a timestream the stages below run on
                self.unstacked[tsconf["name"]] = ts
            else:
                self.timestreams[tsconf["name"]] = ts
            if "simulate" in tsconf:
                self.simulations[tsconf["name"]] = tsconf["simulate"]
            if "stack_from" in tsconf:
                self.stacks[tsconf["name"]] = dict(tsconf["stack_from"])
                self._check_rfi(self.stacks[tsconf["name"]])
            if "sidereal_from" in tsconf:
                self.sidereal[tsconf["name"]] = dict(tsconf["sidereal_from"])
                self._check_rfi(self.sidereal[tsconf["name"]])
        # a stacked day of a `sidereal_from` entry is that entry's input, not a timestream the stages below run on
        daydirs = {os.path.abspath(fixpath(d)) for conf in self.sidereal.values() for d in conf.get("days", ())}
        for name in [n for n, ts in self.timestreams.items() if ts.directory in daydirs]:
            self.days[name] = self.timestreams.pop(name)
        if "crosspower" in yconf:
            self.crosspower = list(yconf["crosspower"] or [])

    @staticmethod
    def _check_rfi(conf):
        """The `rfi`, `rfi_freq`, `rfi_dilate` and `delay` dicts of a `stack_from` or `sidereal_from` block, defaults filled in; an
        unknown key raises ValueError."""
        for key in ("rfi", "rfi_freq"):
            if conf.get(key) is not None:
                conf[key] = timestream.rfi_params(conf[key])
        if conf.get("rfi_dilate") is not None:
            conf["rfi_dilate"] = timestream.rfi_dilate_params(conf["rfi_dilate"])
        if conf.get("delay") is not None:
            conf["delay"] = timestream.delay_params(conf["delay"])

    @staticmethod
    def _rfi_more(conf):
        """The `rfi_freq`, `rfi_dilate` and `delay` keywords of a block, only when present."""
        return {key: conf[key] for key in ("rfi_freq", "rfi_dilate", "delay") if conf.get(key) is not None}

    def _products(self, directory):
        """The ProductManager of a product directory (opened once per directory: its objects hold caches and device
        buffers that the timestreams of one run can share)."""
        cache = self.__dict__.setdefault("_product_cache", {})
        key = fixpath(directory)
        if key not in cache:
            cache[key] = manager.ProductManager.from_config(key)
        self.manager = cache[key] if self.manager is None else self.manager
        return cache[key]

    def simulate(self):
        """Make the timestreams that carry a `simulate` block and do not exist yet."""
        for tsname, simconf in self.simulations.items():
            ts = self.unstacked[tsname] if tsname in self.unstacked else self.timestreams[tsname]
            if os.path.exists(ts._ffile(0)):
                logger.info("Timestream %s exists already, not simulated again.", tsname)
                continue
            simconf = dict(simconf)
            products = self._products(simconf.pop("product_directory", self.product_directory))
            if "maps" in simconf:
                simconf["maps"] = [fixpath(m) for m in simconf["maps"]]
            if "sources" in simconf:
                simconf["sources"] = [fixpath(c) for c in simconf["sources"]]
            if simconf.pop("unstacked", False):
                timestream.simulate_unstacked(products, ts.directory, **simconf)
            else:
                timestream.simulate(products, ts.directory, **simconf)

    @staticmethod
    def _modelcal(conf):
        """The `modelcal` block of a `stack_from` entry: the path of its `model` directory resolved."""
        conf = dict(conf)
        if isinstance(conf.get("model"), str):
            conf["model"] = fixpath(conf["model"])
        return conf

    def stack(self):
        """Make the timestreams that carry a `stack_from` block and whose directory does not exist yet: the unstacked
        directory named there goes through `timestream.stack_baselines`."""
        for tsname, conf in self.stacks.items():
            ts = self.days[tsname] if tsname in self.days else self.timestreams[tsname]
            if os.path.exists(ts.directory):
                logger.info("Timestream %s exists already, not stacked again.", tsname)
                continue
            calibrate = conf.get("calibrate", None)
            timestream.stack_baselines(ts.manager, fixpath(conf["directory"]), ts.directory,
                                       calibrate=None if calibrate in (None, "none") else calibrate,
                                       dead_feeds=tuple(conf.get("dead_feeds", ()) or ()), chunk_gb=self.chunk_gb,
                                       **({"redcal": dict(conf["redcal"])} if conf.get("redcal") else {}),
                                       **({"modelcal": self._modelcal(conf["modelcal"])} if conf.get("modelcal") else {}),
                                       **({"rfi": conf["rfi"]} if conf.get("rfi") is not None else {}), **self._rfi_more(conf))
        # `sidereal_from: {days: [dir, ...], a: 3, min_share: 1.0, rfi: {...}, rfi_freq: {...}, rfi_dilate: {...}}`: the days,
        # which may be the stacks made above, are regridded and averaged by `timestream.sidereal_stack`
        for tsname, conf in self.sidereal.items():
            ts = self.timestreams[tsname]
            if os.path.exists(ts.directory):
                logger.info("Timestream %s exists already, not stacked over its days again.", tsname)
                continue
            timestream.sidereal_stack(ts.manager, [fixpath(d) for d in conf["days"]], ts.directory,
                                      ntime=conf.get("ntime", None), a=int(conf.get("a", 3)),
                                      min_share=float(conf.get("min_share", 1.0)), chunk_gb=self.chunk_gb,
                                      rfi=conf.get("rfi", None), **self._rfi_more(conf))

    def generate(self):
        """Run the stages that are switched on, for every timestream, in the reference's order: m-modes and SVD modes, KL
        modes (collected into one file per filter if `collect_klmodes`), power spectra and cross-power spectra, maps.
        Entries with a `stack_from` block are stacked first, then those with a `sidereal_from` block (`stack`)."""
        self.stack()
        for tsobj in self.timestreams.values():
            os.makedirs(tsobj.output_directory, exist_ok=True)
        if self.generate_modes:
            for tsname, tsobj in self.timestreams.items():
                logger.info("Generating modes (%s)", tsname)
                if self.batched:
                    # the KL filters ride along while the SVD vectors of a batch are on the device
                    tsobj.generate_modes_batched(self.klmodes if self.generate_klmodes else (), chunk_gb=self.chunk_gb)
                else:
                    tsobj.generate_mmodes()
                    tsobj.generate_mmodes_svd()
        if self.generate_klmodes:
            for tsname, tsobj in self.timestreams.items():
                for klname in self.klmodes:
                    logger.info("Generating KL filter (%s:%s)", tsname, klname)
                    tsobj.set_kltransform(klname)
                    if self.batched:
                        tsobj.generate_modes_batched([(klname, tsobj.klthreshold)], chunk_gb=self.chunk_gb)
                    else:
                        tsobj.generate_mmodes_kl()
                    if self.collect_klmodes:
                        tsobj.collect_mmodes_kl()
        if self.generate_powerspectra:
            for tsname, tsobj in self.timestreams.items():
                for ps in self.powerspectra:
                    logger.info("Estimating powerspectra (%s:%s)", tsname, ps["psname"])
                    tsobj.set_kltransform(ps["klname"])
                    tsobj.set_psestimator(ps["psname"])
                    tsobj.powerspectrum()
            for xp in self.crosspower:
                tslist = []
                for tsname in xp["timestreams"]:
                    tsobj = self.timestreams[tsname]
                    tsobj.set_kltransform(xp["klname"])
                    tsobj.set_psestimator(xp["psname"])
                    tslist.append(tsobj)
                timestream.cross_powerspectrum(tslist, xp["psname"], os.path.abspath(fixpath(xp["psfile"])))
        if self.generate_maps:
            for tsname, tsobj in self.timestreams.items():
                for entry in self.ringmaps:
                    entry = timestream.ringmap_params(entry)
                    logger.info("Generating ring map %s (%s)", entry["name"], tsname)
                    timestream.ringmap(tsobj.manager, tsobj.directory, chunk_gb=self.chunk_gb, **entry)
                for entry in self.delayspectra:
                    entry = timestream.delayspectrum_params(entry)
                    logger.info("Generating delay spectrum %s (%s)", entry["name"], tsname)
                    timestream.delay_spectrum(tsobj.manager, tsobj.directory, chunk_gb=self.chunk_gb, **entry)
                for entry in self.formedbeams:
                    entry = timestream.formedbeam_params(entry)
                    logger.info("Forming beams %s (%s)", entry["name"], tsname)
                    timestream.formed_beam(tsobj.manager, tsobj.directory, os.path.abspath(fixpath(entry.pop("catalogue"))),
                                           chunk_gb=self.chunk_gb, **entry)
                for klname in self.klmaps:
                    logger.info("Generating KL map (%s:%s)", tsname, klname)
                    tsobj.set_kltransform(klname)
                    if self.batched:
                        tsobj.mapmake_kl_batched(self.nside, "map_%s.hdf5" % klname, wiener=self.wiener, chunk_gb=self.chunk_gb)
                    else:
                        tsobj.mapmake_kl(self.nside, "map_%s.hdf5" % klname, wiener=self.wiener)
                for entry in self.catalogues:
                    self._catalogue(tsname, tsobj, entry)
                logger.info("Generating SVD map (%s)", tsname)
                if self.batched:
                    tsobj.mapmake_svd_batched(self.nside, "map_svd.hdf5", chunk_gb=self.chunk_gb)
                else:
                    tsobj.mapmake_svd(self.nside, "map_svd.hdf5")
                logger.info("Generating full map (%s)", tsname)
                tsobj.mapmake_full(self.nside, "map_full.hdf5")

    def _catalogue(self, tsname, tsobj, entry):
        """One entry of `catalogues` on one timestream: `Timestream.catalogue_spectra` writes spectra_<name>.hdf5."""
        entry = dict(entry)
        unknown = set(entry) - {"name", "file", "source", "wiener", "stack"}
        if unknown or "name" not in entry or "file" not in entry:
            raise ValueError("catalogues: an entry needs name and file, and may carry source, wiener and stack; got %s"
                             % sorted(entry))
        if not self.batched:
            raise ValueError("catalogues: the spectra at catalogue positions need the batched device route (batched: true)")
        source = entry.get("source", "svd")
        logger.info("Spectra at the positions of %s (%s:%s)", entry["name"], tsname, source)
        if source != "svd":
            tsobj.set_kltransform(source)
        tsobj.catalogue_spectra(fixpath(entry["file"]), source="svd" if source == "svd" else "kl",
                                wiener=bool(entry.get("wiener", self.wiener)), chunk_gb=self.chunk_gb, name=entry["name"],
                                stack=entry.get("stack", None))

    run = generate


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m driftscan_amd.pipeline",
                                     description="Simulate the timestreams that ask for it, then run the pipeline.")
    parser.add_argument("configfile", help="YAML file with `config` and `timestreams` sections")
    args = parser.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    pl = PipelineManager.from_configfile(args.configfile)
    pl.simulate()
    pl.generate()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
