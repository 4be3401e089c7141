DESCRIPTION = "Bfv<UInt32>: the key switch ends in key_switch_finish_kernel instead of in the 4-byte key-MAC transform's store"
EDITS = [("bfv_api.cpp",
          "    const hipError_t fused = heamd::launch_ntt_key_mac_inverse_finish(spread, key, prod, end, image,",
          "    const hipError_t fused = sizeof(W) == 4 ? hipErrorNotSupported : heamd::launch_ntt_key_mac_inverse_finish(spread, key, prod, end, image,")]
