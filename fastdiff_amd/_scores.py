"""The scores of a vocoded waveform against its recording, as infer.py and validate.py offer them: one entry per keyword argument."""
from collections import namedtuple

from . import mcd, pitch, spectral, stoi

# name: the keyword argument, the FastDiff method, the command-line flag and the TSV file; module: its OK / STATUS / RECORD / _enqueue /
# _record; columns: (record key, report and result key, the statuses with which the value counts as measured, TSV format);
# status_key: the status' key in synthesize's report; kwargs(rate, hop): what the method takes besides (clean, degraded, valid);
# config(rate, hop): the sixth argument of module._enqueue, built (and refused) once
Score = namedtuple("Score", "name module columns status_key kwargs config")


def _pitch_config(rate, hop):
    cfg = {"rate": rate, "hop": hop}      # one F0 per mel frame
    pitch.lags(cfg)
    return pitch._config(cfg)


SCORES = (
    Score("stoi", stoi, (("stoi", "stoi", (stoi.OK,), ".6f"), ("estoi", "estoi", (stoi.OK,), ".6f")), "status",
          lambda rate, hop: {"sample_rate": rate}, lambda rate, hop: rate),
    Score("pitch", pitch, (("rmse_cents", "f0_rmse_cents", (pitch.OK,), ".3f"), ("gpe", "gpe", (pitch.OK,), ".6f"),
                           ("vde", "vde", (pitch.OK, pitch.UNVOICED), ".6f")), "pitch_status",
          lambda rate, hop: {"rate": rate, "hop": hop}, _pitch_config),
    Score("spectral", spectral, (("mr_sc", "mr_sc", (spectral.OK,), ".6f"), ("mr_logmag", "mr_logmag", (spectral.OK,), ".6f"),
                                 ("lsd_db", "lsd_db", (spectral.OK,), ".4f")), "spectral_status",
          lambda rate, hop: {}, lambda rate, hop: spectral._config(None)),      # the resolutions are in samples, whatever the rate
    Score("mcd", mcd, (("mcd_dtw", "mcd_dtw", (mcd.OK,), ".4f"), ("mcd_linear", "mcd_linear", (mcd.OK,), ".4f")), "mcd_status",
          lambda rate, hop: {}, lambda rate, hop: mcd._config(None)),           # 13 coefficients of the pwg front-end's frames
)


def enabled(**flags):
    """The entries whose keyword argument is true, in the table's order: enabled(stoi=stoi, pitch=pitch, spectral=spectral, mcd=mcd)."""
    return [s for s in SCORES if flags.get(s.name)]


def refuse(who, advice, **flags):
    """ValueError for the first enabled score, for the entry points that compute none; `advice` may name it as {name}."""
    for s in enabled(**flags):
        raise ValueError(f"{who}: {s.name}=True is not available{advice.format(name=s.name)}")
