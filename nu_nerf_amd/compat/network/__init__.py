"""`network` package of the drop-in (see nu_nerf_amd/compat/__init__.py): this directory provides renderer_zerothick and renderer;
every other `network.*` module is looked up in the `network/` directories further down sys.path -- the user's NU-NeRF checkout.

NU_NERF_DEVICE_METRICS=1 (opt-in) also answers `network.metrics` with nu_nerf_amd.metrics, the device PSNR / SSIM that needs neither
skimage nor cv2; without it network.metrics is the checkout's, like the rest."""
import os
import sys

if os.environ.get('NU_NERF_DEVICE_METRICS') == '1':          # before the checkout's directories can answer the import
    import nu_nerf_amd.metrics as metrics
    sys.modules[__name__ + '.metrics'] = metrics

_here = os.path.dirname(os.path.abspath(__file__))
for _p in list(sys.path):
    _d = os.path.abspath(os.path.join(_p or os.getcwd(), 'network'))
    if os.path.isdir(_d) and _d != _here and _d not in __path__:
        __path__.append(_d)
