# Drop-in replacement for codes/models/modules/discriminator_vgg_arch.py of JingyunLiang/HCFlow (HCFlow+ / ++ recipes):
# networks.define_D / define_F (codes/models/networks.py:44-72) look these classes up by attribute, so every which_model_D
# (discriminator_vgg_128, discriminator_vgg_160, PatchGANDiscriminator) and the feature extractor resolve here.
from hcflow_amd.gan import Discriminator_VGG_128, Discriminator_VGG_160, PatchGANDiscriminator, VGGFeatureExtractor  # noqa: F401
