"""`lora_diffusion.cli_svd` (the reference's `lora_distill` command) resolves to diffusion_finetuning_amd.distill."""
from diffusion_finetuning_amd.distill import _text_lora_path, _ti_lora_path, extract_linear_weights, main, svd_distill  # noqa: F401

if __name__ == "__main__":
    main()
