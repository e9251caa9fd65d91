from .ddim import DDIMScheduler, DDIMSchedulerOutput  # noqa: F401
from .dpm import DPMSolverMultistepScheduler, DPMSolverMultistepSchedulerOutput  # noqa: F401
from .euler import EulerDiscreteScheduler, EulerDiscreteSchedulerOutput  # noqa: F401
from .euler_ancestral import EulerAncestralDiscreteScheduler, EulerAncestralDiscreteSchedulerOutput  # noqa: F401
from .lcm import LCMScheduler, LCMSchedulerOutput  # noqa: F401
from .unipc import UniPCMultistepScheduler, UniPCMultistepSchedulerOutput  # noqa: F401
