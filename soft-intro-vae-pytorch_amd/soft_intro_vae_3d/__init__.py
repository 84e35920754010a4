"""Drop-in modules for the reference's soft_intro_vae_3d/ (put this directory first on PYTHONPATH): `models.vae`,
`losses.chamfer_loss` and `metrics.jsd` with the reference's names, signatures and state_dict keys, on the HIP kernels of
sivae_hip."""
