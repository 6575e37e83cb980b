"""fastdiff_amd -- MI355X-native FastDiff vocoder inference path (denoiser + N-step reverse sampler).

Drop-in names of the reference:
    fastdiff_amd.FastDiff                          <- modules.FastDiff.module.FastDiff_model.FastDiff
    fastdiff_amd.sampler (alias fastdiff_amd.util): sampling_given_noise_schedule, compute_hyperparams_given_schedule, noise_scheduling, theta_timestep_loss (under no_grad and under autograd), phi_loss, ...
                                                   <- modules.FastDiff.module.util
    fastdiff_amd.location_variable_convolution     <- TimeAware_LVCBlock.location_variable_convolution (modules.py:220-253), forward AND backward
FastDiff.forward in train() mode records an autograd graph (fastdiff_amd/train.py) whose LVC nodes are that operator;
fastdiff_amd.TrainStep runs a whole training step -- draws, loss, clip, AdamW included -- as one graph replay (fastdiff_amd/trainstep.py),
fed from a device-resident fastdiff_amd.TrainCorpus whose batches are cut inside that replay (fastdiff_amd/corpus.py);
fastdiff_amd.Validator runs a held-out pass on the device over fixed draws, with the loss per noise level (fastdiff_amd/validate.py);
fastdiff_amd.ParamEMA keeps an exponential moving average of the parameters on the device, updated inside TrainStep's replay, and
FastDiff.use_weights lets the inference kernels compute from it (fastdiff_amd/ema.py);
fastdiff_amd.NoisePredictor is a scheduling network of this project's own design (the reference ships none), fastdiff_amd.PhiStep trains it
on the device against the frozen denoiser, and noise_scheduling(..., search="device") derives a short schedule from it without a host
round trip per iteration (fastdiff_amd/noisepred.py, phistep.py);
FastDiff.sample_long / stream vocode one utterance of any length window by window, FastDiff.sample_long_batch / stream_pool
(fastdiff_amd.StreamPool) many utterances or live streams in shared window batches (fastdiff_amd/longform.py);
fastdiff_amd.resample / FastDiff.resample convert sample rate, sample type and channel count on the device, so recordings of any rate
feed the mel front-end and TrainCorpus.from_wav_dir, and infer.synthesize writes PCM at any rate (fastdiff_amd/resample.py);
fastdiff_amd.loudness / FastDiff.loudness / loudness_normalize measure BS.1770 loudness and normalise to a target on the device: the
reference's loud_norm in front of the mel, and infer.synthesize(loudness=-23) behind the vocoder (fastdiff_amd/loudness.py);
fastdiff_amd.stoi / FastDiff.stoi score a vocoded waveform against its recording with STOI and ESTOI on the device, Validator(stoi=True)
does so for every held-out window and infer.synthesize(stoi=True) / --stoi in copy synthesis (fastdiff_amd/stoi.py);
fastdiff_amd.pitch / FastDiff.pitch track F0 with YIN on the mel frame grid and score the vocoded pitch against the recording's (F0 RMSE in
cents, gross pitch error, voicing decision error), Validator(pitch=True) and infer.synthesize(pitch=True) / --pitch likewise
(fastdiff_amd/pitch.py);
fastdiff_amd.spectral / FastDiff.spectral measure the multi-resolution STFT distances (spectral convergence, log-magnitude distance,
log-spectral distance) of the vocoded spectrum against the recording's, Validator(spectral=True) and infer.synthesize(spectral=True) /
--spectral likewise (fastdiff_amd/spectral.py);
fastdiff_amd.mcd / FastDiff.mcd measure the mel-cepstral distortion of a vocoded waveform against its recording, along a time-warped path
(dynamic time warping on the device: mcd.dtw) and frame by frame, Validator(mcd=True) and infer.synthesize(mcd=True) / --mcd likewise
(fastdiff_amd/mcd.py);
fastdiff_amd.trim / FastDiff.trim_silences cut the long silences of a recording on the device -- the reference's trim_long_sil, with an energy
detector in place of WebRTC's -- and infer.load_wav_inputs(trim_long_sil=True) / --trim_long_sil and TrainCorpus.from_wav_dir(trim_long_sil=True)
put it in front of the mel (fastdiff_amd/trim.py);
fastdiff_amd.griffin_lim / FastDiff.griffin_lim / mel_to_linear / griffin_lim_mel are the baseline vocoder (the reference's GLLinear /
GLMel) with its inverse STFT on the device and both mel inversions (the pseudo-inverse, which is the default, and GLMel's non-negative
least squares: mel_to_linear(inversion="nnls"), griffin_lim.mel_to_linear_nnls), and infer.synthesize_griffin_lim / --vocoder griffin_lim put its rows next to the model's
(fastdiff_amd/griffin_lim.py);
fastdiff_amd.diversity fits k-means bins over the corpus' mel frames on the device (TrainCorpus.fit_bins) and scores a whole run against
them with NDB and JSD, the paper's two diversity columns; infer --ndb_bins writes the row (fastdiff_amd/diversity.py).
"""
from .model import FastDiff  # noqa: F401
from . import sampler, schedules, resample, loudness, stoi, pitch, spectral, mcd, trim, griffin_lim, diversity, pwg  # noqa: F401
from . import sampler as util  # noqa: F401  (the reference module is called util)
from .lvc_op import location_variable_convolution, gated_residual, kernel_conv1d, conv32  # noqa: F401
from .trainstep import TrainStep  # noqa: F401
from .corpus import TrainCorpus  # noqa: F401
from .validate import Validator  # noqa: F401
from .ema import ParamEMA  # noqa: F401
from .noisepred import NoisePredictor  # noqa: F401
from .phistep import PhiStep  # noqa: F401
from .longform import StreamPool, SampleStream  # noqa: F401
from .sampler import (compute_hyperparams_given_schedule, sampling_given_noise_schedule, noise_scheduling,  # noqa: F401
                   map_noise_scale_to_time_step, calc_diffusion_step_embedding, std_normal, theta_timestep_loss, phi_loss, calc_diffusion_hyperparams)

__all__ = ["FastDiff", "TrainStep", "TrainCorpus", "Validator", "ParamEMA", "NoisePredictor", "PhiStep", "StreamPool", "SampleStream", "location_variable_convolution", "gated_residual", "kernel_conv1d", "conv32", "util", "schedules", "resample", "loudness", "stoi", "pitch", "spectral", "mcd", "trim", "griffin_lim", "diversity", "pwg", "compute_hyperparams_given_schedule", "sampling_given_noise_schedule",
           "noise_scheduling", "map_noise_scale_to_time_step", "calc_diffusion_step_embedding", "std_normal", "theta_timestep_loss", "phi_loss", "calc_diffusion_hyperparams"]
