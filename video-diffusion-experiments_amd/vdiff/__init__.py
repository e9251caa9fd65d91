"""vdiff — MI355X-native video-diffusion denoising step (AnimateDiff UNetMotionModel + DDIM / Euler).

Host mirror of the reference's call surface (diffusers UNetMotionModel /
DDIMScheduler / AnimateDiffPipeline as used by tanm-ast/video-diffusion-
experiments) over hand-written gfx950 HIP kernels in libvdiff_hip.so.
"""
from .config import FULL, TINY, get_config  # noqa: F401
from .models import UNetMotionModel, UNetMotionOutput  # noqa: F401
from .models.controlnet import ControlNetModel, ControlNetOutput  # noqa: F401
from .models.sparse_controlnet import SparseControlNetModel  # noqa: F401
from .models.clip import CLIPTextModel, CLIPTextModelOutput  # noqa: F401
from .models.clip import CLIPVisionModelWithProjection, ImageProjection  # noqa: F401
from .image_processor import CLIPImageProcessor  # noqa: F401
from .models.dit import DiT3DModel, DiTDenoiseLoop, DiTOutput  # noqa: F401
from .models.vae import (AutoencoderKL, AutoencoderKLOutput, DecoderOutput,  # noqa: F401
                         DiagonalGaussianDistribution)
from .pretrained import MotionAdapter  # noqa: F401
from .pipeline import (AnimateDiffControlNetPipeline, AnimateDiffPAGPipeline, AnimateDiffPipeline,  # noqa: F401
                       AnimateDiffPipelineOutput, AnimateDiffSparseControlNetPipeline,
                       AnimateDiffVideoToVideoPipeline, ControlNetConditioning, DenoiseLoop,
                       PerturbedAttentionGuidance, SparseControlConditioning)
from .sched import (DDIMScheduler, DDIMSchedulerOutput, DPMSolverMultistepScheduler,  # noqa: F401
                    DPMSolverMultistepSchedulerOutput, EulerAncestralDiscreteScheduler,
                    EulerAncestralDiscreteSchedulerOutput, EulerDiscreteScheduler, EulerDiscreteSchedulerOutput,
                    LCMScheduler, LCMSchedulerOutput, UniPCMultistepScheduler, UniPCMultistepSchedulerOutput)
from .tokenizer import CLIPTokenizer  # noqa: F401
from .weights import init_synthetic_, load_diffusers_state_dict  # noqa: F401
