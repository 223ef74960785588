"""ace355: MI355X-native (gfx950) ACE-Step 1.5 denoise + decode hot path.

Layout:
  csrc/        hand-written HIP kernels + the C-ABI shared library (include/ace355.h)
  native.py    ctypes binding of the C-ABI (fails loudly when the library is missing)
  dit.py       NativeDit: weight packing, condition slots, forward, sampler
  vae.py       NativeVae: weight-norm fusion, decode
  cond.py      NativeCondEncoder: lyric / timbre encoders + sequence packing
  lmhints.py   audio-code parsing, FSQ index decode, NativeDetokenizer
  textenc.py   NativeTextEncoder: the caption text encoder (Qwen3Model, causal) and its embed_tokens gather
  lm.py        NativeCausalLM: the 5 Hz LM's forward (Qwen3ForCausalLM): prefill, KV-cached decode steps, last-position logits
  lmsample.py  select_tokens / filter_logits_: top-k, top-p and the draw on the LM's logits in one native call
  lmlogits.py  shape_logits / SeenTokens / step_plan / generate_with_cfg: the LM's logits stage and its device-resident CFG loop
  lmscore.py   calculate_pmi_score_per_condition and its helpers: the reference's LM quality score on NativeCausalLM.score
  audio_out.py normalize_audio, AudioSaver: GPU normalise / PCM conversion + threaded FLAC / WAV writers
  audio_in.py  load_stereo_48k, reference_segments: WAV / FLAC payload -> clamped 48 kHz stereo on the GPU (the producer of row N3);
               decode_flac: a FLAC file's frames decoded on the GPU, 16 to 24 bits (opt-in)
  backend.py   NativeDitMixin / NativeVaeMixin / NativeHandler: the reference's handler seam
  dist.py      one-process-per-GPU data-parallel runner (RCCL broadcast of conditioning)
  weightgen.py deterministic synthetic weights (no checkpoints exist on the boxes)
"""
from .config import CondConfig, DetokConfig, DitConfig, LmConfig, TextEncoderConfig, VaeConfig  # noqa: F401

__all__ = ["CondConfig", "DetokConfig", "DitConfig", "LmConfig", "TextEncoderConfig", "VaeConfig"]
